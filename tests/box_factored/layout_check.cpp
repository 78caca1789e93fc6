// The box factor buffer's layout (csrc/qpb_factor.h, bxfct) and its route
// (csrc/qpb_route.h, route_box_factored), host only: including the two headers
// compiles their static_asserts; main() walks n = 1..34 and checks that the
// sections tile the buffer in order, each on a 16-byte boundary, that the class
// changes where the route's kernel does, and that the route ends where the
// layout's limit does.
#include <cstdio>

#include "qpb_factor.h"
#include "qpb_route.h"

static int fails = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s (n=%d)\n", __LINE__, #cond, n);  \
      ++fails;                                                  \
    }                                                           \
  } while (0)

int main() {
  using namespace qpb;
  for (int n = 1; n <= 34; ++n) {
    const bxfct::Layout y = bxfct::layout(n);
    const Route r = route_box_factored(n);
    CHECK(y.box16 == (n <= 16));
    CHECK(y.np == (n <= 16 ? 16 : 32));
    const long long lsize = y.box16 ? 16 * 16 : 32 * 33 / 2;
    CHECK(y.L == bxfct::kHdr && y.D == y.L + lsize && y.dn2 == y.D + (long long)y.np * y.np &&
          y.size == y.dn2 + y.np);
    CHECK(y.L % 2 == 0 && y.D % 2 == 0 && y.dn2 % 2 == 0 && y.size % 2 == 0);
    if (n <= bxfct::kMaxN) {
      CHECK(r.step > 0);
      CHECK((r.kernel == Kernel::gi_box) == y.box16);
      CHECK(r.kernel == route(n, 2 * n, 0, true).kernel && r.step == route(n, 2 * n, 0, true).step);
      CHECK(r.kernel == route_bwd_box_shared(n).kernel);
      // smaller than the general buffer of the explicit A = [I; -I]: no H, no A, one row of D per variable
      CHECK(y.size < fct::layout(n, 2 * n).size);
    } else {
      CHECK(r.step == 0);
    }
  }
  if (fails) return 1;
  std::printf("layout_check ok\n");
  return 0;
}
