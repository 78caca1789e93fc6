// plan_check.cpp -- TEST INFRASTRUCTURE ONLY: the slice plan of the batch sum
// (qpb::sum_plan, csrc/qpb_route.h), host only, in the manner of
// tests/route/route_check.cpp.  For batches 1 .. 5000 and a few up to 2^40:
// the slices tile the batch (every QP lies in exactly one), every slice starts
// at a multiple of 4 and is at least one QP long, all but the last hold `per`
// QPs, per is a multiple of 4 and at least kSumMinSlice, and the slot count
// stays within kSumMaxSlots.  With arguments it prints "slots per" for each
// batch given (tests/test_shared_plan.py compares qpb.sum_plan with it).
#include <cstdio>
#include <cstdlib>

#include "qpb_route.h"

static int check(long long batch) {
  const qpb::SumPlan p = qpb::sum_plan(batch);
  auto bad = [&](const char *what) {
    std::printf("batch %lld: slots %lld per %lld: %s\n", batch, p.slots, p.per, what);
    return 1;
  };
  if (p.slots < 1 || p.slots > qpb::kSumMaxSlots) return bad("slot count outside 1 .. kSumMaxSlots");
  if (p.per < qpb::kSumMinSlice || p.per % 4 != 0) return bad("per is not a multiple of 4 of at least kSumMinSlice");
  // slice s = [s per, min(batch, (s + 1) per)): consecutive by construction, so
  // they tile the batch iff the last one is non-empty and ends at `batch`
  if ((p.slots - 1) * p.per >= batch) return bad("an empty last slice");
  if (p.slots * p.per < batch) return bad("QPs past the last slice");
  if (batch <= 5000) {  // and QP by QP
    long long covered = 0;
    for (long long s = 0; s < p.slots; ++s) {
      const long long kb = s * p.per, ke = kb + p.per < batch ? kb + p.per : batch;
      if (kb % 4 != 0) return bad("a slice start that is no multiple of 4");
      if (kb != covered || ke <= kb) return bad("a gap, an overlap or an empty slice");
      covered = ke;
    }
    if (covered != batch) return bad("the slices do not end at the batch");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1) {
    for (int i = 1; i < argc; ++i) {
      const qpb::SumPlan p = qpb::sum_plan(std::atoll(argv[i]));
      std::printf("%lld %lld\n", p.slots, p.per);
    }
    return 0;
  }
  int failed = 0;
  for (long long b = 1; b <= 5000; ++b) failed += check(b);
  const long long big[] = {65536,      131071,     131072,       131073,       262144,      1048576,
                           1048577,    (1LL << 27), (1LL << 31) - 1, (1LL << 31) + 5, (1LL << 40) - 3, 1LL << 40};
  for (long long b : big) failed += check(b);
  if (qpb::sum_plan(0).slots != 0 || qpb::sum_plan(-1).slots != 0) {
    std::printf("an empty batch has slices\n");
    ++failed;
  }
  if (failed) return 1;
  std::printf("plan_check ok\n");
  return 0;
}
