// route_multi_check.cpp -- stand-alone host check of the routes of
// qpb_solve_factored_backward_multi and qpb_solve_box_backward_multi in
// csrc/qpb_route.h (tests/test_route_backward_multi.py builds it with the host
// compiler under ASan + UBSan and runs it).  Including the header compiles its
// static_asserts; the loops below hold the two routes to the single-direction
// calls whose bits they promise, over every size, and walk the chunks the way
// qpb_api.hip does: the right-hand sides and outputs advance by T n and T m per
// QP, the right-hand sides by 0 with QPB_SHARED_RHS.
#include "qpb_route.h"

#include <cstdio>
#include <vector>

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

struct Chunk {
  long long count;
  const double *fac, *gx, *glam;
  const unsigned *act;
  double *gf, *gb;
};

// the chunk walk of the factored call (the box call's has H, stride 0 or n n, in bfac's place)
static void walk(long long B, long long step, long long n, long long m, long long T, bool shared_rhs) {
  const long long rs = shared_rhs ? 0 : T, words = (m + 31) / 32;
  std::vector<double> fac(4), gx((shared_rhs ? 1 : B) * T * n), glam((shared_rhs ? 1 : B) * T * m), gf(B * T * n),
      gb(B * T * m);
  std::vector<unsigned> act(B * words);
  const int *no_status = nullptr;
  std::vector<Chunk> seen;
  const int rc = qpb::for_each_chunk(
      B, step,
      [&](long long count, const double *Fc, const unsigned *ac, const int *sc, const double *gxc, const double *glc,
          double *gfc, double *gbc) {
        CHECK(sc == nullptr, "status NULL stays NULL");
        seen.push_back({count, Fc, gxc, glc, ac, gfc, gbc});
        return 0;
      },
      qpb::required((const double *)fac.data(), 0), qpb::optional((const unsigned *)act.data(), words),
      qpb::optional(no_status, 1), qpb::required((const double *)gx.data(), rs * n),
      qpb::optional((const double *)glam.data(), rs * m), qpb::optional(gf.data(), T * n),
      qpb::optional(gb.data(), T * m));
  CHECK(rc == 0, "rc=%d", rc);
  CHECK((long long)seen.size() == (B + step - 1) / step, "B=%lld step=%lld chunks=%zu", B, step, seen.size());
  long long k0 = 0;
  for (const Chunk &c : seen) {
    CHECK(c.count == (B - k0 < step ? B - k0 : step), "B=%lld k0=%lld count=%lld", B, k0, c.count);
    CHECK(c.fac == fac.data(), "the buffer does not move");
    CHECK(c.act == act.data() + k0 * words, "active at k0=%lld", k0);
    CHECK(c.gx == gx.data() + k0 * rs * n && c.glam == glam.data() + k0 * rs * m,
          "right-hand sides at k0=%lld T=%lld shared=%d", k0, T, (int)shared_rhs);
    CHECK(c.gf == gf.data() + k0 * T * n && c.gb == gb.data() + k0 * T * m, "outputs at k0=%lld T=%lld", k0, T);
    if (shared_rhs) CHECK(c.gx == gx.data() && c.glam == glam.data(), "one set for every chunk");
    // the chunk's last direction ends inside the arrays
    CHECK(c.gf + c.count * T * n <= gf.data() + gf.size() && c.gb + c.count * T * m <= gb.data() + gb.size(),
          "outputs end at k0=%lld", k0);
    if (!shared_rhs) CHECK(c.gx + c.count * T * n <= gx.data() + gx.size(), "gx ends at k0=%lld", k0);
    k0 += c.count;
  }
  CHECK(k0 == B, "covered %lld of %lld", k0, B);
}

int main() {
  for (int n = 1; n <= 129; ++n)
    for (int m = 0; m <= 257; ++m) {
      const qpb::Route d = qpb::route_factored_bwd_multi(n, m);
      const qpb::Route f = qpb::route_factored_bwd_dual(n, m), b = qpb::route_factored_bwd(n, m);
      // each direction's bits are the single-direction calls' on the same buffer
      CHECK(d.kernel == f.kernel && d.step == f.step, "n=%d m=%d", n, m);
      CHECK(d.kernel == b.kernel && d.step == b.step, "n=%d m=%d", n, m);
      const bool in = n <= 32 && m <= 64;
      CHECK((d.step > 0) == in, "n=%d m=%d step=%lld", n, m, d.step);
      CHECK(in == (n <= qpb::kBwdMultiMaxN && m <= qpb::kBwdMultiMaxM), "n=%d m=%d", n, m);
      if (in) CHECK((d.kernel == qpb::Kernel::gi_dense) == (n <= 16 && m <= 32), "n=%d m=%d", n, m);
    }
  for (int n = 1; n <= 129; ++n) {
    const qpb::Route d = qpb::route_bwd_box_multi(n);
    const qpb::Route u = qpb::route_bwd_box_dual(n), b = qpb::route_bwd_box(n), s = qpb::route_bwd_box_shared(n);
    CHECK(d.kernel == u.kernel && d.step == u.step, "n=%d", n);
    CHECK(d.kernel == b.kernel && d.step == b.step, "n=%d", n);
    CHECK(d.kernel == s.kernel && d.step == s.step, "n=%d", n);
    CHECK((d.step > 0) == (n <= 32), "n=%d step=%lld", n, d.step);
    CHECK((n <= 32) == (n <= qpb::kBwdBoxMultiMaxN), "n=%d", n);
    if (d.step > 0) CHECK((d.kernel == qpb::Kernel::gi_box) == (n <= 16), "n=%d", n);
  }
  CHECK(qpb::kMaxRhs == 256, "kMaxRhs=%d", qpb::kMaxRhs);
  // the walk, with small steps in the routes' place: whole, ragged and single chunks
  for (long long T : {1LL, 2LL, 5LL, 17LL})
    for (int sh = 0; sh < 2; ++sh) {
      walk(67, 16, 16, 32, T, sh != 0);
      walk(67, 67, 5, 3, T, sh != 0);
      walk(64, 16, 20, 40, T, sh != 0);
      walk(5, 1, 3, 0, T, sh != 0);
      walk(1, 1LL << 27, 32, 64, T, sh != 0);
    }
  if (failures) {
    std::printf("route_multi_check: %d failures\n", failures);
    return 1;
  }
  std::printf("route_multi_check ok\n");
  return 0;
}
