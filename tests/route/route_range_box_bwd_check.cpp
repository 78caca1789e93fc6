// route_range_box_bwd_check.cpp -- stand-alone host check of
// qpb_solve_range_box_backward's route in csrc/qpb_route.h
// (tests/test_route_range_box_bwd.py builds it with the host compiler under
// ASan + UBSan and runs it).  Including the header compiles its static_asserts;
// the loop below holds the route to route_bwd_dual of the materialised shape,
// its classes and its limit, over every size, not only at the classes' corners.
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
    for (int mg = 0; mg <= 257; ++mg) {
      const qpb::Route b = qpb::route_bwd_range_box(n, mg);
      // the bits are qpb_solve_backward_dual's on [G; I]: that call's class and step
      const qpb::Route r = qpb::route_bwd_dual(n, mg + n);
      CHECK(b.kernel == r.kernel && b.step == r.step, "n=%d mg=%d", n, mg);
      const bool in = n <= qpb::kBwdRangeBoxMaxN && mg + n <= qpb::kBwdRangeBoxMaxRows;
      CHECK((b.step > 0) == in, "n=%d mg=%d step=%lld", n, mg, b.step);
      CHECK(in == (n <= 32 && mg + n <= 64), "n=%d mg=%d", n, mg);
      if (in) {
        const bool dense = n <= 16 && mg + n <= 32;
        CHECK((b.kernel == qpb::Kernel::gi_dense) == dense, "n=%d mg=%d", n, mg);
        CHECK((b.kernel == qpb::Kernel::gi_wave) == !dense, "n=%d mg=%d", n, mg);
        CHECK(b.step == qpb::step_of(b.kernel), "n=%d mg=%d step=%lld", n, mg, b.step);
        // without glam and with nothing shared the call on [G; I] is qpb_solve_backward, with a
        // shared operand qpb_solve_shared_backward: the same class and chunks
        const qpb::Route p = qpb::route_bwd(n, mg + n), s = qpb::route_shared_bwd(n, mg + n);
        CHECK(p.kernel == b.kernel && p.step == b.step, "n=%d mg=%d", n, mg);
        CHECK(s.kernel == b.kernel && s.step == b.step, "n=%d mg=%d", n, mg);
        // every solve of qpb_solve_range_box has this backward, in the forward's class
        CHECK(qpb::route_range_box(n, mg).step > 0 && qpb::route_range_box(n, mg).kernel == b.kernel, "n=%d mg=%d",
              n, mg);
      } else {
        CHECK(qpb::route_range_box(n, mg).step == 0, "n=%d mg=%d", n, mg);
      }
    }
  if (failures) {
    std::printf("route_range_box_bwd_check: %d failures\n", failures);
    return 1;
  }
  std::printf("route_range_box_bwd_check ok\n");
  return 0;
}
