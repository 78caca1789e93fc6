// qpb_route.h -- which kernel a problem shape goes to, how many QPs one launch
// of it takes, and the walk of a batch in such chunks.  Host-only plain C++:
// no HIP header, so the host compiler builds it alone (tests/route/).
#pragma once

#include "qpb.h"  // QPB_FLAG_MIXED, QPB_FLAG_DIAG_WAVE

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
