// qpb_route.h -- which kernel a problem shape goes to, how many QPs one launch
// of it takes, and the walk of a batch in such chunks.  Host-only plain C++:
// no HIP header, so the host compiler builds it alone (tests/route/).
#pragma once

#include "qpb.h"  // QPB_FLAG_MIXED, QPB_FLAG_DIAG_WAVE
#include "qpb_factor.h"  // bxfct: the box factor buffer's class boundary (host-compilable as well)

namespace qpb {

enum class Kernel { gi_dense, gi_wave, gi_mixed, gi_gram, gi_box, gi_wave_box, gi_gram_box };

// QPs per launch: a launch's grid holds at most 2^32 - 1 work-items, so a
// kernel takes at most 2^32 / (threads per QP) QPs per launch (minus a
// margin); larger batches are split into consecutive launches on the stream.
constexpr long long step_of(Kernel k) {
  switch (k) {
    case Kernel::gi_dense: return 1LL << 27;     // 16 lanes per QP
    case Kernel::gi_box: return 1LL << 27;
    case Kernel::gi_wave: return 1LL << 25;      // 64 lanes per QP
    case Kernel::gi_mixed: return 1LL << 25;
    case Kernel::gi_wave_box: return 1LL << 25;
    case Kernel::gi_gram: return 1LL << 21;      // one workgroup per CU walks the QPs (bounded chunks)
    case Kernel::gi_gram_box: return 1LL << 25;  // not gi_gram's, for compatibility; a later pull request may reconcile
  }
  return 0;
}

struct Route {
  Kernel kernel;
  long long step;  // QPs per launch
};

// n <= 16, m <= 32: four QPs per wavefront; n <= 32, m <= 64: one QP per
// wavefront; larger (n <= QPB_MAX_N, m <= QPB_MAX_M): one QP per workgroup.
// box: qpb_solve_box, m = 2n implicit, flags select nothing.
constexpr Route route(int n, int m, int flags, bool box) {
  Kernel k = Kernel::gi_gram;
  if (box)
    k = n <= 16 ? Kernel::gi_box : n <= 32 ? Kernel::gi_wave_box : Kernel::gi_gram_box;
  else if (n <= 16 && m <= 32 && !(flags & QPB_FLAG_DIAG_WAVE))
    k = Kernel::gi_dense;
  else if (n <= 32 && m <= 64)
    k = (n > 16 && (flags & QPB_FLAG_MIXED)) ? Kernel::gi_mixed : Kernel::gi_wave;
  return {k, step_of(k)};
}

static_assert(route(16, 32, 0, false).kernel == Kernel::gi_dense);
static_assert(route(16, 33, 0, false).kernel == Kernel::gi_wave);
static_assert(route(17, 1, 0, false).kernel == Kernel::gi_wave);
static_assert(route(32, 64, 0, false).kernel == Kernel::gi_wave);
static_assert(route(32, 65, 0, false).kernel == Kernel::gi_gram);
static_assert(route(33, 0, 0, false).kernel == Kernel::gi_gram);
static_assert(route(128, 256, 0, false).kernel == Kernel::gi_gram);
static_assert(route(7, 14, QPB_FLAG_DIAG_WAVE, false).kernel == Kernel::gi_wave);
static_assert(route(16, 32, QPB_FLAG_MIXED, false).kernel == Kernel::gi_dense);
static_assert(route(20, 33, QPB_FLAG_MIXED, false).kernel == Kernel::gi_mixed);
static_assert(route(16, 32, QPB_FLAG_MIXED | QPB_FLAG_DIAG_WAVE, false).kernel == Kernel::gi_wave);
static_assert(route(1, 2, 0, true).kernel == Kernel::gi_box);
static_assert(route(16, 32, 0, true).kernel == Kernel::gi_box);
static_assert(route(17, 34, 0, true).kernel == Kernel::gi_wave_box);
static_assert(route(32, 64, 0, true).kernel == Kernel::gi_wave_box);
static_assert(route(33, 66, 0, true).kernel == Kernel::gi_gram_box);
static_assert(route(128, 256, 0, true).kernel == Kernel::gi_gram_box);
static_assert(route(16, 32, QPB_FLAG_MIXED | QPB_FLAG_DIAG_WAVE, true).kernel == Kernel::gi_box);
static_assert(route(20, 40, QPB_FLAG_MIXED, true).kernel == Kernel::gi_wave_box);
static_assert(step_of(Kernel::gi_dense) == 1LL << 27 && step_of(Kernel::gi_wave) == 1LL << 25 &&
              step_of(Kernel::gi_mixed) == 1LL << 25 && step_of(Kernel::gi_gram) == 1LL << 21);
static_assert(step_of(Kernel::gi_box) == 1LL << 27 && step_of(Kernel::gi_wave_box) == 1LL << 25 &&
              step_of(Kernel::gi_gram_box) == 1LL << 25);
static_assert(route(32, 65, 0, false).step == 1LL << 21 && route(33, 66, 0, true).step == 1LL << 25);

// qpb_solve_eq with meq > 0: the EQ forms of the two wavefront-level classes,
// whatever the flags (the call accepts none).  Above them -- the n <= 128 Gram
// class -- there is no EQ form yet: step 0, and the call is unsupported.
constexpr Route route_eq(int n, int m) {
  if (n <= 16 && m <= 32) return {Kernel::gi_dense, step_of(Kernel::gi_dense)};
  if (n <= 32 && m <= 64) return {Kernel::gi_wave, step_of(Kernel::gi_wave)};
  return {Kernel::gi_gram, 0};
}
constexpr int kEqMaxN = 32, kEqMaxM = 64;  // the limit route_eq's step 0 stands for

static_assert(route_eq(16, 32).kernel == Kernel::gi_dense && route_eq(1, 1).kernel == Kernel::gi_dense);
static_assert(route_eq(16, 33).kernel == Kernel::gi_wave && route_eq(17, 1).kernel == Kernel::gi_wave);
static_assert(route_eq(32, 64).kernel == Kernel::gi_wave && route_eq(32, 64).step == 1LL << 25);
static_assert(route_eq(16, 32).step == 1LL << 27);
static_assert(route_eq(33, 0).step == 0 && route_eq(32, 65).step == 0 && route_eq(16, 65).step == 0 &&
              route_eq(128, 256).step == 0);
static_assert(route_eq(kEqMaxN, kEqMaxM).step > 0 && route_eq(kEqMaxN + 1, 1).step == 0 &&
              route_eq(1, kEqMaxM + 1).step == 0);

// qpb_solve_backward: the two wavefront-level classes of qpb_kkt_bwd.hip,
// named by the forward kernel whose lane mapping they share; above them there
// is no backward kernel yet: step 0, and the call is unsupported.
constexpr Route route_bwd(int n, int m) {
  if (n <= 16 && m <= 32) return {Kernel::gi_dense, step_of(Kernel::gi_dense)};
  if (n <= 32 && m <= 64) return {Kernel::gi_wave, step_of(Kernel::gi_wave)};
  return {Kernel::gi_gram, 0};
}
constexpr int kBwdMaxN = 32, kBwdMaxM = 64;  // the limit route_bwd's step 0 stands for

static_assert(route_bwd(16, 32).kernel == Kernel::gi_dense && route_bwd(1, 0).kernel == Kernel::gi_dense);
static_assert(route_bwd(16, 33).kernel == Kernel::gi_wave && route_bwd(17, 0).kernel == Kernel::gi_wave);
static_assert(route_bwd(32, 64).kernel == Kernel::gi_wave && route_bwd(32, 64).step == 1LL << 25);
static_assert(route_bwd(16, 32).step == 1LL << 27);
static_assert(route_bwd(33, 0).step == 0 && route_bwd(32, 65).step == 0 && route_bwd(128, 256).step == 0);
static_assert(route_bwd(kBwdMaxN, kBwdMaxM).step > 0 && route_bwd(kBwdMaxN + 1, 1).step == 0 &&
              route_bwd(1, kBwdMaxM + 1).step == 0);

// qpb_solve_box_backward: the two wavefront-level classes of qpb_kkt_bwd_box.hip,
// named by the forward box kernel whose lane mapping they share (m = 2n
// implicit); above them there is no backward kernel yet: step 0, and the call
// is unsupported.
constexpr Route route_bwd_box(int n) {
  if (n <= 16) return {Kernel::gi_box, step_of(Kernel::gi_box)};
  if (n <= 32) return {Kernel::gi_wave_box, step_of(Kernel::gi_wave_box)};
  return {Kernel::gi_gram_box, 0};
}
constexpr int kBwdBoxMaxN = 32;  // the limit route_bwd_box's step 0 stands for

static_assert(route_bwd_box(1).kernel == Kernel::gi_box && route_bwd_box(16).kernel == Kernel::gi_box);
static_assert(route_bwd_box(17).kernel == Kernel::gi_wave_box && route_bwd_box(32).kernel == Kernel::gi_wave_box);
static_assert(route_bwd_box(16).step == 1LL << 27 && route_bwd_box(32).step == 1LL << 25);
static_assert(route_bwd_box(33).step == 0 && route_bwd_box(128).step == 0);
static_assert(route_bwd_box(kBwdBoxMaxN).step > 0 && route_bwd_box(kBwdBoxMaxN + 1).step == 0);
// the backward of a box solve runs wherever the forward's own class does, up to the limit
static_assert(route_bwd_box(16).kernel == route(16, 32, 0, true).kernel &&
              route_bwd_box(17).kernel == route(17, 34, 0, true).kernel);

// qpb_solve_box_shared: qpb_solve_box's own route at every shape it takes -- each
// of the three box kernels has an SH form; qpb_solve_box_shared_backward:
// route_bwd_box, with its limit.
constexpr Route route_box_shared(int n) { return route(n, 2 * n, 0, true); }
constexpr Route route_bwd_box_shared(int n) { return route_bwd_box(n); }

static_assert(route_box_shared(1).kernel == Kernel::gi_box && route_box_shared(16).kernel == Kernel::gi_box);
static_assert(route_box_shared(17).kernel == Kernel::gi_wave_box && route_box_shared(32).kernel == Kernel::gi_wave_box);
static_assert(route_box_shared(33).kernel == Kernel::gi_gram_box && route_box_shared(128).kernel == Kernel::gi_gram_box);
// both name the unshared call's class and step
static_assert(route_box_shared(16).kernel == route(16, 32, 0, true).kernel &&
              route_box_shared(16).step == route(16, 32, 0, true).step &&
              route_box_shared(32).kernel == route(32, 64, 0, true).kernel &&
              route_box_shared(32).step == route(32, 64, 0, true).step &&
              route_box_shared(128).kernel == route(128, 256, 0, true).kernel &&
              route_box_shared(128).step == route(128, 256, 0, true).step);
static_assert(route_bwd_box_shared(16).kernel == route_bwd_box(16).kernel &&
              route_bwd_box_shared(16).step == route_bwd_box(16).step &&
              route_bwd_box_shared(32).kernel == route_bwd_box(32).kernel &&
              route_bwd_box_shared(32).step == route_bwd_box(32).step &&
              route_bwd_box_shared(kBwdBoxMaxN + 1).step == 0);

// qpb_factor_box and qpb_solve_box_factored: qpb_solve_box's own two
// wavefront-level classes, whose factor kernel writes and whose factored form
// reads the class's own layout of the box buffer (qpb_factor.h, bxfct, decides
// the class by the same limit); above them -- the Gram class, whose set-up runs
// on the matrix cores -- there is neither yet: step 0, and the calls are
// unsupported.
constexpr Route route_box_factored(int n) {
  if (n <= 16) return {Kernel::gi_box, step_of(Kernel::gi_box)};
  if (n <= 32) return {Kernel::gi_wave_box, step_of(Kernel::gi_wave_box)};
  return {Kernel::gi_gram_box, 0};
}
constexpr int kBoxFactoredMaxN = 32;  // the limit route_box_factored's step 0 stands for

static_assert(route_box_factored(1).kernel == Kernel::gi_box && route_box_factored(16).kernel == Kernel::gi_box);
static_assert(route_box_factored(17).kernel == Kernel::gi_wave_box &&
              route_box_factored(32).kernel == Kernel::gi_wave_box);
static_assert(route_box_factored(16).step == 1LL << 27 && route_box_factored(32).step == 1LL << 25);
static_assert(route_box_factored(33).step == 0 && route_box_factored(128).step == 0);
static_assert(route_box_factored(kBoxFactoredMaxN).step > 0 && route_box_factored(kBoxFactoredMaxN + 1).step == 0);
// up to the limit it names qpb_solve_box's class and step
static_assert(route_box_factored(1).kernel == route(1, 2, 0, true).kernel &&
              route_box_factored(16).kernel == route(16, 32, 0, true).kernel &&
              route_box_factored(16).step == route(16, 32, 0, true).step &&
              route_box_factored(17).kernel == route(17, 34, 0, true).kernel &&
              route_box_factored(32).kernel == route(32, 64, 0, true).kernel &&
              route_box_factored(32).step == route(32, 64, 0, true).step);
// the buffer's layout changes class where the route does, and ends where it does
static_assert(bxfct::layout(1).box16 == (route_box_factored(1).kernel == Kernel::gi_box) &&
              bxfct::layout(16).box16 == (route_box_factored(16).kernel == Kernel::gi_box) &&
              bxfct::layout(17).box16 == (route_box_factored(17).kernel == Kernel::gi_box) &&
              bxfct::layout(32).box16 == (route_box_factored(32).kernel == Kernel::gi_box) &&
              bxfct::kMaxN == kBoxFactoredMaxN);
// the outputs go to qpb_solve_box_shared_backward: the same classes and limit
static_assert(route_box_factored(16).kernel == route_bwd_box_shared(16).kernel &&
              route_box_factored(17).kernel == route_bwd_box_shared(17).kernel &&
              kBoxFactoredMaxN == kBwdBoxMaxN);

// qpb_solve_shared with a shared H or A (and any meq): route_eq, the SH forms
// of the two wavefront-level classes; above them -- the Gram class -- there is
// no shared form yet: step 0, and the call is unsupported.
constexpr Route route_shared(int n, int m) {
  const Route r = route_eq(n, m);
  return {r.kernel, r.step};
}
// qpb_solve_shared_backward with a shared H or A: route_bwd in the same way
constexpr Route route_shared_bwd(int n, int m) {
  const Route r = route_bwd(n, m);
  return {r.kernel, r.step};
}
constexpr int kSharedMaxN = 32, kSharedMaxM = 64;  // the limit the two routes' step 0 stands for

static_assert(route_shared(16, 32).kernel == Kernel::gi_dense && route_shared(1, 0).kernel == Kernel::gi_dense);
static_assert(route_shared(16, 33).kernel == Kernel::gi_wave && route_shared(32, 64).kernel == Kernel::gi_wave);
static_assert(route_shared(16, 32).step == 1LL << 27 && route_shared(32, 64).step == 1LL << 25);
static_assert(route_shared(33, 0).step == 0 && route_shared(32, 65).step == 0 && route_shared(128, 256).step == 0);
static_assert(route_shared_bwd(16, 32).kernel == Kernel::gi_dense && route_shared_bwd(17, 0).kernel == Kernel::gi_wave);
static_assert(route_shared_bwd(16, 32).step == 1LL << 27 && route_shared_bwd(32, 64).step == 1LL << 25);
static_assert(route_shared_bwd(33, 0).step == 0 && route_shared_bwd(32, 65).step == 0);
static_assert(route_shared(kSharedMaxN, kSharedMaxM).step > 0 && route_shared(kSharedMaxN + 1, 1).step == 0 &&
              route_shared(1, kSharedMaxM + 1).step == 0);
static_assert(route_shared_bwd(kSharedMaxN, kSharedMaxM).step > 0 && route_shared_bwd(kSharedMaxN + 1, 1).step == 0 &&
              route_shared_bwd(1, kSharedMaxM + 1).step == 0);

// qpb_solve_backward_dual: route_shared_bwd's classes, whose DU forms (plain and
// SH) take glam; above them there is none: step 0, and the call is unsupported.
constexpr Route route_bwd_dual(int n, int m) {
  const Route r = route_shared_bwd(n, m);
  return {r.kernel, r.step};
}
constexpr int kBwdDualMaxN = kSharedMaxN, kBwdDualMaxM = kSharedMaxM;

static_assert(route_bwd_dual(1, 0).kernel == Kernel::gi_dense && route_bwd_dual(16, 32).kernel == Kernel::gi_dense);
static_assert(route_bwd_dual(16, 33).kernel == Kernel::gi_wave && route_bwd_dual(17, 0).kernel == Kernel::gi_wave &&
              route_bwd_dual(32, 64).kernel == Kernel::gi_wave);
static_assert(route_bwd_dual(16, 32).kernel == route_shared_bwd(16, 32).kernel &&
              route_bwd_dual(16, 32).step == route_shared_bwd(16, 32).step &&
              route_bwd_dual(32, 64).kernel == route_shared_bwd(32, 64).kernel &&
              route_bwd_dual(32, 64).step == route_shared_bwd(32, 64).step);
static_assert(route_bwd_dual(33, 0).step == 0 && route_bwd_dual(16, 65).step == 0 && route_bwd_dual(129, 32).step == 0);
static_assert(route_bwd_dual(kBwdDualMaxN, kBwdDualMaxM).step > 0 && route_bwd_dual(kBwdDualMaxN + 1, 1).step == 0 &&
              route_bwd_dual(1, kBwdDualMaxM + 1).step == 0);

// qpb_factor_shared and qpb_solve_factored: route_shared's classes, whose
// factor kernel writes and whose factored form reads the class's own layout of
// the buffer (qpb_factor.h decides the class by the same two limits); above
// them there is neither: step 0, and the calls are unsupported.
constexpr Route route_factored(int n, int m) {
  const Route r = route_shared(n, m);
  return {r.kernel, r.step};
}
constexpr int kFactoredMaxN = kSharedMaxN, kFactoredMaxM = kSharedMaxM;

static_assert(route_factored(16, 32).kernel == Kernel::gi_dense && route_factored(1, 0).kernel == Kernel::gi_dense);
static_assert(route_factored(16, 33).kernel == Kernel::gi_wave && route_factored(17, 0).kernel == Kernel::gi_wave &&
              route_factored(32, 64).kernel == Kernel::gi_wave);
static_assert(route_factored(16, 32).step == 1LL << 27 && route_factored(32, 64).step == 1LL << 25);
static_assert(route_factored(33, 0).step == 0 && route_factored(16, 65).step == 0 && route_factored(128, 256).step == 0);
static_assert(route_factored(kFactoredMaxN, kFactoredMaxM).step > 0 && route_factored(kFactoredMaxN + 1, 1).step == 0 &&
              route_factored(1, kFactoredMaxM + 1).step == 0);

// qpb_factor_shared_backward and qpb_solve_factored_backward: route_shared_bwd's
// classes, whose factor form writes and whose factored form reads the class's
// own layout of the backward's buffer (qpb_factor.h, bfct, decides the class by
// the same two limits); above them there is neither: step 0, and the calls are
// unsupported.
constexpr Route route_factored_bwd(int n, int m) {
  const Route r = route_shared_bwd(n, m);
  return {r.kernel, r.step};
}
constexpr int kFactoredBwdMaxN = kSharedMaxN, kFactoredBwdMaxM = kSharedMaxM;

static_assert(route_factored_bwd(16, 32).kernel == Kernel::gi_dense &&
              route_factored_bwd(1, 0).kernel == Kernel::gi_dense);
static_assert(route_factored_bwd(16, 33).kernel == Kernel::gi_wave &&
              route_factored_bwd(17, 0).kernel == Kernel::gi_wave &&
              route_factored_bwd(32, 64).kernel == Kernel::gi_wave);
static_assert(route_factored_bwd(16, 32).step == 1LL << 27 && route_factored_bwd(32, 64).step == 1LL << 25);
static_assert(route_factored_bwd(33, 0).step == 0 && route_factored_bwd(16, 65).step == 0 &&
              route_factored_bwd(128, 256).step == 0);
static_assert(route_factored_bwd(kFactoredBwdMaxN, kFactoredBwdMaxM).step > 0 &&
              route_factored_bwd(kFactoredBwdMaxN + 1, 1).step == 0 &&
              route_factored_bwd(1, kFactoredBwdMaxM + 1).step == 0);
// a factored forward's outputs go to the factored backward: the same classes and limits
static_assert(route_factored_bwd(16, 32).kernel == route_factored(16, 32).kernel &&
              route_factored_bwd(16, 33).kernel == route_factored(16, 33).kernel &&
              route_factored_bwd(17, 0).kernel == route_factored(17, 0).kernel &&
              kFactoredBwdMaxN == kFactoredMaxN && kFactoredBwdMaxM == kFactoredMaxM);

// qpb_solve_factored_backward_dual: route_factored_bwd's classes, whose DU forms
// of the factored forms take glam on the same buffer; above them there is
// none: step 0, and the call is unsupported.
constexpr Route route_factored_bwd_dual(int n, int m) {
  const Route r = route_factored_bwd(n, m);
  return {r.kernel, r.step};
}
constexpr int kFactoredBwdDualMaxN = kFactoredBwdMaxN, kFactoredBwdDualMaxM = kFactoredBwdMaxM;

static_assert(route_factored_bwd_dual(1, 0).kernel == Kernel::gi_dense &&
              route_factored_bwd_dual(16, 32).kernel == Kernel::gi_dense);
static_assert(route_factored_bwd_dual(16, 33).kernel == Kernel::gi_wave &&
              route_factored_bwd_dual(17, 0).kernel == Kernel::gi_wave &&
              route_factored_bwd_dual(32, 64).kernel == Kernel::gi_wave);
// the buffer is the factored backward's and the bits are the unfactored dual call's: both classes and steps
static_assert(route_factored_bwd_dual(16, 32).kernel == route_factored_bwd(16, 32).kernel &&
              route_factored_bwd_dual(16, 32).step == route_factored_bwd(16, 32).step &&
              route_factored_bwd_dual(32, 64).kernel == route_factored_bwd(32, 64).kernel &&
              route_factored_bwd_dual(32, 64).step == route_factored_bwd(32, 64).step);
static_assert(route_factored_bwd_dual(16, 32).kernel == route_bwd_dual(16, 32).kernel &&
              route_factored_bwd_dual(16, 33).kernel == route_bwd_dual(16, 33).kernel &&
              route_factored_bwd_dual(17, 0).kernel == route_bwd_dual(17, 0).kernel &&
              route_factored_bwd_dual(16, 32).step == route_bwd_dual(16, 32).step &&
              route_factored_bwd_dual(32, 64).step == route_bwd_dual(32, 64).step);
static_assert(route_factored_bwd_dual(33, 0).step == 0 && route_factored_bwd_dual(16, 65).step == 0 &&
              route_factored_bwd_dual(128, 256).step == 0);
static_assert(route_factored_bwd_dual(kFactoredBwdDualMaxN, kFactoredBwdDualMaxM).step > 0 &&
              route_factored_bwd_dual(kFactoredBwdDualMaxN + 1, 1).step == 0 &&
              route_factored_bwd_dual(1, kFactoredBwdDualMaxM + 1).step == 0);
static_assert(kFactoredBwdDualMaxN == kBwdDualMaxN && kFactoredBwdDualMaxM == kBwdDualMaxM);

// qpb_solve_box_backward_dual, batched H or one H: route_bwd_box's classes,
// whose DU forms (plain and SH) take glam; above them there is none: step 0,
// and the call is unsupported.
constexpr Route route_bwd_box_dual(int n) { return route_bwd_box(n); }
constexpr int kBwdBoxDualMaxN = kBwdBoxMaxN;

static_assert(route_bwd_box_dual(1).kernel == Kernel::gi_box && route_bwd_box_dual(16).kernel == Kernel::gi_box);
static_assert(route_bwd_box_dual(17).kernel == Kernel::gi_wave_box &&
              route_bwd_box_dual(32).kernel == Kernel::gi_wave_box);
static_assert(route_bwd_box_dual(16).kernel == route_bwd_box_shared(16).kernel &&
              route_bwd_box_dual(16).step == route_bwd_box_shared(16).step &&
              route_bwd_box_dual(32).kernel == route_bwd_box_shared(32).kernel &&
              route_bwd_box_dual(32).step == route_bwd_box_shared(32).step);
static_assert(route_bwd_box_dual(33).step == 0 && route_bwd_box_dual(128).step == 0);
static_assert(route_bwd_box_dual(kBwdBoxDualMaxN).step > 0 && route_bwd_box_dual(kBwdBoxDualMaxN + 1).step == 0);
// a box solve's outputs go to it unchanged: the forward's classes
static_assert(route_bwd_box_dual(16).kernel == route(16, 32, 0, true).kernel &&
              route_bwd_box_dual(17).kernel == route(17, 34, 0, true).kernel);

// qpb_solve_factored_backward_multi and qpb_solve_box_backward_multi: the
// single-direction dual routes' classes, whose MU forms loop over T right-hand
// sides per QP, and their steps (a chunk is `step` QPs whatever T is: the
// kernels' grids count QPs); above them there is none: step 0, and the calls
// are unsupported.
constexpr Route route_factored_bwd_multi(int n, int m) {
  const Route r = route_factored_bwd_dual(n, m);
  return {r.kernel, r.step};
}
constexpr Route route_bwd_box_multi(int n) { return route_bwd_box_dual(n); }
constexpr int kBwdMultiMaxN = kFactoredBwdDualMaxN, kBwdMultiMaxM = kFactoredBwdDualMaxM;
constexpr int kBwdBoxMultiMaxN = kBwdBoxDualMaxN;
constexpr int kMaxRhs = 256;  // QPB_MAX_RHS: every column of K^-1 at the largest shape in one call

static_assert(route_factored_bwd_multi(1, 0).kernel == Kernel::gi_dense &&
              route_factored_bwd_multi(16, 32).kernel == Kernel::gi_dense);
static_assert(route_factored_bwd_multi(16, 33).kernel == Kernel::gi_wave &&
              route_factored_bwd_multi(17, 0).kernel == Kernel::gi_wave &&
              route_factored_bwd_multi(32, 64).kernel == Kernel::gi_wave);
// each direction's bits are the single-direction call's on the same buffer: its classes and steps
static_assert(route_factored_bwd_multi(16, 32).kernel == route_factored_bwd_dual(16, 32).kernel &&
              route_factored_bwd_multi(16, 32).step == route_factored_bwd_dual(16, 32).step &&
              route_factored_bwd_multi(32, 64).kernel == route_factored_bwd_dual(32, 64).kernel &&
              route_factored_bwd_multi(32, 64).step == route_factored_bwd_dual(32, 64).step);
static_assert(route_factored_bwd_multi(33, 0).step == 0 && route_factored_bwd_multi(16, 65).step == 0 &&
              route_factored_bwd_multi(128, 256).step == 0);
static_assert(route_factored_bwd_multi(kBwdMultiMaxN, kBwdMultiMaxM).step > 0 &&
              route_factored_bwd_multi(kBwdMultiMaxN + 1, 1).step == 0 &&
              route_factored_bwd_multi(1, kBwdMultiMaxM + 1).step == 0);
static_assert(route_bwd_box_multi(1).kernel == Kernel::gi_box && route_bwd_box_multi(16).kernel == Kernel::gi_box);
static_assert(route_bwd_box_multi(17).kernel == Kernel::gi_wave_box &&
              route_bwd_box_multi(32).kernel == Kernel::gi_wave_box);
static_assert(route_bwd_box_multi(16).kernel == route_bwd_box_dual(16).kernel &&
              route_bwd_box_multi(16).step == route_bwd_box_dual(16).step &&
              route_bwd_box_multi(32).kernel == route_bwd_box_dual(32).kernel &&
              route_bwd_box_multi(32).step == route_bwd_box_dual(32).step);
static_assert(route_bwd_box_multi(33).step == 0 && route_bwd_box_multi(128).step == 0);
static_assert(route_bwd_box_multi(kBwdBoxMultiMaxN).step > 0 && route_bwd_box_multi(kBwdBoxMultiMaxN + 1).step == 0);
// every column of K^-1 in one call: n + m right-hand sides at the largest shape
static_assert(kMaxRhs >= kBwdMultiMaxN + kBwdMultiMaxM && kMaxRhs >= 3 * kBwdBoxMultiMaxN);
// a chunk's largest element offset, step QPs of kMaxRhs directions of m doubles, is far inside 63 bits
static_assert(route_factored_bwd_multi(16, 32).step <= (1LL << 62) / (kMaxRhs * kBwdMultiMaxM));

// qpb_solve_range with m > 0: the RG forms of the two wavefront-level classes,
// whatever meq and the shared bits (the forms take both at run time); above
// them -- the Gram class -- there is no range form yet: step 0, and the call is
// unsupported.
constexpr Route route_range(int n, int m) {
  if (n <= 16 && m <= 32) return {Kernel::gi_dense, step_of(Kernel::gi_dense)};
  if (n <= 32 && m <= 64) return {Kernel::gi_wave, step_of(Kernel::gi_wave)};
  return {Kernel::gi_gram, 0};
}
constexpr int kRangeMaxN = 32, kRangeMaxM = 64;  // the limit route_range's step 0 stands for

static_assert(route_range(16, 32).kernel == Kernel::gi_dense && route_range(1, 1).kernel == Kernel::gi_dense);
static_assert(route_range(16, 33).kernel == Kernel::gi_wave && route_range(17, 1).kernel == Kernel::gi_wave);
static_assert(route_range(32, 64).kernel == Kernel::gi_wave && route_range(32, 64).step == 1LL << 25);
static_assert(route_range(16, 32).step == 1LL << 27);
static_assert(route_range(33, 1).step == 0 && route_range(32, 65).step == 0 && route_range(1, 65).step == 0 &&
              route_range(128, 256).step == 0);
static_assert(route_range(kRangeMaxN, kRangeMaxM).step > 0 && route_range(kRangeMaxN + 1, 1).step == 0 &&
              route_range(1, kRangeMaxM + 1).step == 0);
// a range solve's outputs go to qpb_solve_backward unchanged: the same classes
static_assert(route_range(16, 32).kernel == route_bwd(16, 32).kernel &&
              route_range(32, 64).kernel == route_bwd(32, 64).kernel);
// qpb_solve_range_factored goes by route_factored (the buffer's layout is the
// class's): it names route_range's class, and its step, at the classes' corners
static_assert(route_factored(1, 1).kernel == route_range(1, 1).kernel &&
              route_factored(16, 32).kernel == route_range(16, 32).kernel &&
              route_factored(16, 33).kernel == route_range(16, 33).kernel &&
              route_factored(17, 1).kernel == route_range(17, 1).kernel &&
              route_factored(32, 64).kernel == route_range(32, 64).kernel);
static_assert(route_factored(16, 32).step == route_range(16, 32).step &&
              route_factored(32, 64).step == route_range(32, 64).step && route_factored(33, 1).step == 0 &&
              route_factored(1, 65).step == 0);
static_assert(kFactoredMaxN == kRangeMaxN && kFactoredMaxM == kRangeMaxM);

// qpb_solve_range_box, mg general rows beside the n variables' bounds: the range
// route of the materialised problem's shape, m' = mg + n rows -- the BX forms of
// the RG forms sit in its two classes, lane for lane -- and its limit: step 0
// above it, and the call is unsupported.  mg == 0 is a shape of its own here
// (qpb_solve_range hands m == 0 to qpb_solve).
constexpr Route route_range_box(int n, int mg) { return route_range(n, mg + n); }
constexpr int kRangeBoxMaxN = kRangeMaxN, kRangeBoxMaxRows = kRangeMaxM;  // n, and mg + n

static_assert(route_range_box(16, 16).kernel == Kernel::gi_dense && route_range_box(16, 17).kernel == Kernel::gi_wave &&
              route_range_box(12, 20).kernel == Kernel::gi_dense);
static_assert(route_range_box(32, 32).kernel == Kernel::gi_wave && route_range_box(32, 32).step == 1LL << 25);
static_assert(route_range_box(32, 33).step == 0 && route_range_box(33, 0).step == 0);
static_assert(route_range_box(1, 0).kernel == Kernel::gi_dense && route_range_box(16, 0).kernel == Kernel::gi_dense &&
              route_range_box(17, 0).kernel == Kernel::gi_wave && route_range_box(16, 16).step == 1LL << 27);
static_assert(route_range_box(kRangeBoxMaxN, kRangeBoxMaxRows - kRangeBoxMaxN).step > 0 &&
              route_range_box(kRangeBoxMaxN + 1, 0).step == 0 && route_range_box(1, kRangeBoxMaxRows).step == 0);
// its bits are qpb_solve_range's on [G; I]: that call's class and step at every corner
static_assert(route_range_box(16, 16).kernel == route_range(16, 32).kernel &&
              route_range_box(16, 16).step == route_range(16, 32).step &&
              route_range_box(16, 17).kernel == route_range(16, 33).kernel &&
              route_range_box(32, 32).kernel == route_range(32, 64).kernel &&
              route_range_box(32, 32).step == route_range(32, 64).step);

// qpb_solve_range_box_backward: the backward route of the materialised problem's
// shape, m' = mg + n rows, with or without glam and shared operands -- the BX
// forms sit in route_bwd_dual's two classes, and the call's bits are that
// call's on [G; I] only in the same class and with the same chunks.
constexpr Route route_bwd_range_box(int n, int mg) { return route_bwd_dual(n, mg + n); }
constexpr int kBwdRangeBoxMaxN = kBwdDualMaxN, kBwdRangeBoxMaxRows = kBwdDualMaxM;  // n, and mg + n

static_assert(route_bwd_range_box(16, 16).kernel == Kernel::gi_dense &&
              route_bwd_range_box(16, 17).kernel == Kernel::gi_wave &&
              route_bwd_range_box(12, 20).kernel == Kernel::gi_dense &&
              route_bwd_range_box(1, 0).kernel == Kernel::gi_dense &&
              route_bwd_range_box(16, 0).kernel == Kernel::gi_dense &&
              route_bwd_range_box(17, 0).kernel == Kernel::gi_wave &&
              route_bwd_range_box(32, 32).kernel == Kernel::gi_wave);
static_assert(route_bwd_range_box(16, 16).step == route_bwd_dual(16, 32).step &&
              route_bwd_range_box(32, 32).step == route_bwd_dual(32, 64).step &&
              route_bwd_range_box(16, 16).step == route_bwd(16, 32).step &&
              route_bwd_range_box(32, 32).step == route_shared_bwd(32, 64).step);
static_assert(route_bwd_range_box(33, 0).step == 0 && route_bwd_range_box(32, 33).step == 0 &&
              route_bwd_range_box(16, 49).step == 0 && route_bwd_range_box(129, 32).step == 0);
static_assert(route_bwd_range_box(kBwdRangeBoxMaxN, kBwdRangeBoxMaxRows - kBwdRangeBoxMaxN).step > 0 &&
              route_bwd_range_box(kBwdRangeBoxMaxN + 1, 0).step == 0 &&
              route_bwd_range_box(1, kBwdRangeBoxMaxRows).step == 0);
// every solve of qpb_solve_range_box has a backward, in the forward's class
static_assert(kBwdRangeBoxMaxN == kRangeBoxMaxN && kBwdRangeBoxMaxRows == kRangeBoxMaxRows &&
              route_bwd_range_box(16, 16).kernel == route_range_box(16, 16).kernel &&
              route_bwd_range_box(16, 17).kernel == route_range_box(16, 17).kernel &&
              route_bwd_range_box(32, 32).kernel == route_range_box(32, 32).kernel);

// The slice plan of the batch sum (qpb_kkt_bwd_sum.hip): `slots` consecutive
// slices of `per` QPs, the last one shorter; one wavefront and one workspace
// slot per slice.  A function of the batch size alone -- not of the device --
// so that the summed gradients' bits are reproducible anywhere.  per is a
// multiple of 4 (a wave takes 4 QPs per matrix-core step), at least
// kSumMinSlice (a shorter slice leaves the finish kernel more slots to add
// than the wave saved), and large enough for at most kSumMaxSlots slices
// (four waves on each of 256 CUs; the slots are the finish kernel's input).
struct SumPlan {
  long long slots;  // slices, each with a slot of sum_slot_doubles(n, m) doubles
  long long per;    // QPs per slice
};
constexpr long long kSumMaxSlots = 1024, kSumMinSlice = 128;
constexpr SumPlan sum_plan(long long batch) {
  if (batch <= 0) return {0, 0};
  long long per = (batch + kSumMaxSlots - 1) / kSumMaxSlots;
  if (per < kSumMinSlice) per = kSumMinSlice;
  per = (per + 3) / 4 * 4;
  return {(batch + per - 1) / per, per};
}
// a slot: S as 16 ceil(n/16) squared, then gA's sum as 16 ceil(m/16) x 16 ceil(n/16)
constexpr long long sum_slot_doubles(int n, int m) {
  const long long nt = (n + 15) / 16, mt = (m + 15) / 16;
  return 256 * (nt * nt + mt * nt);
}

static_assert(kSumMinSlice % 4 == 0 && kSumMinSlice > 0 && kSumMaxSlots > 0);
static_assert(sum_plan(0).slots == 0 && sum_plan(1).slots == 1 && sum_plan(1).per == kSumMinSlice);
static_assert(sum_plan(kSumMinSlice).slots == 1 && sum_plan(kSumMinSlice + 1).slots == 2);
static_assert(sum_plan(kSumMaxSlots * kSumMinSlice).slots == kSumMaxSlots &&
              sum_plan(kSumMaxSlots * kSumMinSlice).per == kSumMinSlice);
static_assert(sum_plan(kSumMaxSlots * kSumMinSlice + 1).slots <= kSumMaxSlots &&
              sum_plan(kSumMaxSlots * kSumMinSlice + 1).per == kSumMinSlice + 4);
static_assert(sum_plan(1LL << 20).slots == 1024 && sum_plan(1LL << 20).per == 1024);
static_assert(sum_plan(1LL << 40).slots <= kSumMaxSlots && sum_plan(1LL << 40).per % 4 == 0 &&
              sum_plan(1LL << 40).slots * sum_plan(1LL << 40).per >= 1LL << 40 &&
              (sum_plan(1LL << 40).slots - 1) * sum_plan(1LL << 40).per < 1LL << 40);
static_assert(sum_slot_doubles(16, 32) == 768 && sum_slot_doubles(32, 64) == 3072 && sum_slot_doubles(1, 0) == 256 &&
              sum_slot_doubles(17, 33) == 256 * (4 + 6));

// One array of a batched call: per_qp elements per QP from base.  Only an
// optional array may be NULL, and then it is NULL in every chunk.
template <class T>
struct Batched {
  T *base;
  long long per_qp;
  bool optional;
  constexpr T *at(long long k0) const { return optional && !base ? nullptr : base + k0 * per_qp; }
};
template <class T>
constexpr Batched<T> required(T *base, long long per_qp) {
  return {base, per_qp, false};
}
template <class T>
constexpr Batched<T> optional(T *base, long long per_qp) {
  return {base, per_qp, true};
}

// Walks `batch` QPs in chunks of at most `step`: f(count, pointers...) once per
// chunk with each array advanced to the chunk's first QP.  Stops at the first
// nonzero return of f and returns it; batch <= 0 makes no call.
template <class F, class... T>
constexpr int for_each_chunk(long long batch, long long step, F &&f, Batched<T>... arrays) {
  for (long long k0 = 0; k0 < batch; k0 += step) {
    const long long count = batch - k0 < step ? batch - k0 : step;
    if (const int rc = f(count, arrays.at(k0)...)) return rc;
  }
  return 0;
}

}  // namespace qpb
