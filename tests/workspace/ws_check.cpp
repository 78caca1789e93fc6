// ws_check.cpp -- the workspace cache of csrc/qpb_workspace.hip on the host,
// without a GPU: the unmodified source, compiled host-only, linked against the
// stub definitions below of the six HIP calls it makes.  Its own main; built
// under ThreadSanitizer and under AddressSanitizer + UBSan and run directly
// (tests/test_workspace_host.py).
//
// The stubs back hipMallocAsync / hipFreeAsync with malloc / free and a
// mutex-guarded set of live buffers that remembers the device and stream each
// was allocated on: a free of a pointer that is not live, on another stream or
// with another device current aborts.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

hipError_t qpb_with_workspace(hipStream_t stream, size_t bytes, const std::function<hipError_t(void *)> &launch);
extern "C" int qpb_release_stream_workspace(void *stream);
extern "C" int qpb_release_workspaces(void);

namespace {
struct Live {
  size_t bytes;
  int dev;
  hipStream_t stream;
};
std::mutex g_live_mu;
std::map<void *, Live> g_live;
thread_local int t_dev = 0;
std::atomic<int> g_fail_mallocs{0};  // the next so many hipMallocAsync calls fail
std::atomic<long> g_mallocs{0}, g_frees{0}, g_syncs{0};

[[noreturn]] void die(const char *what, const void *p) {
  std::fprintf(stderr, "ws_check stub: %s (%p)\n", what, p);
  std::abort();
}

size_t live_count() {
  std::lock_guard<std::mutex> l(g_live_mu);
  return g_live.size();
}
// bytes of the live buffer at p, 0 if p is not live
size_t live_bytes(void *p) {
  std::lock_guard<std::mutex> l(g_live_mu);
  auto it = g_live.find(p);
  return it == g_live.end() ? 0 : it->second.bytes;
}

int g_failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                         \
    }                                                                       \
  } while (0)

hipStream_t fake_stream(uintptr_t v) { return reinterpret_cast<hipStream_t>(v); }
constexpr size_t MiB = 1u << 20;
}  // namespace

// ---- the six HIP calls of qpb_workspace.hip ----------------------------------
extern "C" hipError_t hipGetDevice(int *dev) {
  *dev = t_dev;
  return hipSuccess;
}
extern "C" hipError_t hipSetDevice(int dev) {
  t_dev = dev;
  return hipSuccess;
}
extern "C" hipError_t hipMallocAsync(void **p, size_t bytes, hipStream_t stream) {
  int left = g_fail_mallocs.load();
  while (left > 0 && !g_fail_mallocs.compare_exchange_weak(left, left - 1)) {
  }
  if (left > 0) {
    *p = reinterpret_cast<void *>(0xdead0);  // a failed call leaves nothing to free
    return hipErrorOutOfMemory;
  }
  void *q = std::malloc(bytes);
  if (!q) return hipErrorOutOfMemory;
  {
    std::lock_guard<std::mutex> l(g_live_mu);
    g_live[q] = Live{bytes, t_dev, stream};
  }
  ++g_mallocs;
  *p = q;
  return hipSuccess;
}
extern "C" hipError_t hipFreeAsync(void *p, hipStream_t stream) {
  {
    std::lock_guard<std::mutex> l(g_live_mu);
    auto it = g_live.find(p);
    if (it == g_live.end()) die("free of a pointer that is not live", p);
    if (it->second.stream != stream) die("free on another stream than the allocation's", p);
    if (it->second.dev != t_dev) die("free with another device current than the allocation's", p);
    g_live.erase(it);
  }
  std::free(p);
  ++g_frees;
  return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_syncs;
  return hipSuccess;
}

namespace {
// One call: the callback must run exactly once, with a live buffer of at least
// `bytes`, whose first and last requested byte it writes.  Returns the buffer.
void *call(hipStream_t s, size_t bytes, size_t *size = nullptr) {
  void *got = nullptr;
  int runs = 0;
  const hipError_t e = qpb_with_workspace(s, bytes, [&](void *p) {
    ++runs;
    got = p;
    const size_t have = live_bytes(p);
    CHECK(have >= bytes);
    if (size) *size = have;
    if (have >= bytes && bytes) {
      static_cast<volatile unsigned char *>(p)[0] = 0x5a;
      static_cast<volatile unsigned char *>(p)[bytes - 1] = 0xa5;
    }
    return hipSuccess;
  });
  CHECK(e == hipSuccess);
  CHECK(runs == 1);
  return got;
}

void check_identity() {
  const hipStream_t s1 = fake_stream(0x1000), s2 = fake_stream(0x2000), null_stream = nullptr;
  size_t sz = 0;
  void *a = call(s1, 100, &sz);
  CHECK(a && sz == MiB);  // rounded up to 1 MiB
  CHECK(live_count() == 1);
  CHECK(call(s1, 100) == a);  // no growth: the same buffer
  CHECK(call(s1, MiB) == a);
  CHECK(call(s1, 1) == a);
  const long frees = g_frees;
  void *a2 = call(s1, MiB + 1, &sz);  // growth: the old buffer is freed, on s1
  CHECK(a2 && sz == 2 * MiB && g_frees == frees + 1);
  CHECK(live_count() == 1);
  CHECK(call(s1, 7) == a2);  // never shrinks
  void *b = call(s2, 100);
  CHECK(b != a2 && live_count() == 2);  // streams do not share
  void *c = call(null_stream, 3 * MiB - 5, &sz);
  CHECK(c != a2 && c != b && sz == 3 * MiB && live_count() == 3);
  CHECK(call(s1, 2 * MiB) == a2 && call(s2, MiB) == b);
  // the callback's error is the call's, and the buffer stays cached
  CHECK(qpb_with_workspace(s2, 10, [](void *) { return hipErrorInvalidValue; }) == hipErrorInvalidValue);
  CHECK(call(s2, 10) == b);
  // the same stream handle on another device: another buffer
  CHECK(hipSetDevice(1) == hipSuccess);
  void *d = call(s1, 100);
  CHECK(d != a2 && live_count() == 4);
  CHECK(call(s1, 100) == d);
  CHECK(hipSetDevice(0) == hipSuccess);
  CHECK(call(s1, 100) == a2);
  // releasing s1 frees its buffer on both devices (each with its device
  // current, or the stub aborts), waits for the stream and restores the device
  const long syncs = g_syncs;
  CHECK(qpb_release_stream_workspace(s1) == 0);
  int dev = -1;
  CHECK(hipGetDevice(&dev) == hipSuccess && dev == 0);
  CHECK(live_count() == 2 && live_bytes(a2) == 0 && live_bytes(d) == 0 && live_bytes(b) && live_bytes(c));
  CHECK(g_syncs == syncs + 2);
  CHECK(qpb_release_stream_workspace(s1) == 0);                  // nothing left: success
  CHECK(qpb_release_stream_workspace(fake_stream(0x7000)) == 0);  // never used: success
  CHECK(live_count() == 2);
  call(s1, 100, &sz);  // usable again after the release
  CHECK(sz == MiB && live_count() == 3);
  CHECK(qpb_release_workspaces() == 0);
  CHECK(live_count() == 0);
  CHECK(qpb_release_workspaces() == 0);  // twice in a row
  CHECK(g_mallocs == g_frees);
}

void check_alloc_failure() {
  const hipStream_t s = fake_stream(0x3000);
  int runs = 0;
  auto cb = [&](void *) {
    ++runs;
    return hipSuccess;
  };
  // the first allocation of a stream fails
  g_fail_mallocs = 1;
  CHECK(qpb_with_workspace(s, 100, cb) == hipErrorOutOfMemory);
  CHECK(runs == 0 && live_count() == 0 && g_fail_mallocs == 0);
  void *a = call(s, 100);
  CHECK(a && live_count() == 1);
  // growing fails: the old buffer is gone (freed once), nothing is cached
  g_fail_mallocs = 1;
  CHECK(qpb_with_workspace(s, MiB + 1, cb) == hipErrorOutOfMemory);
  CHECK(runs == 0 && live_count() == 0);
  size_t sz = 0;
  void *b = call(s, 100, &sz);  // the next call allocates afresh
  CHECK(b && sz == MiB && live_count() == 1);
  // a release after a failed growth frees nothing twice
  g_fail_mallocs = 1;
  CHECK(qpb_with_workspace(s, 2 * MiB + 1, cb) == hipErrorOutOfMemory);
  CHECK(qpb_release_stream_workspace(s) == 0);
  CHECK(live_count() == 0);
  call(s, 100);
  CHECK(qpb_release_workspaces() == 0);
  CHECK(live_count() == 0 && g_mallocs == g_frees && runs == 0);
}

// Six threads over three streams, two per stream, 2 000 calls each.  The
// callback writes the buffer and a per-stream counter without any lock of its
// own: the cache's entry lock is what orders the two threads of a stream (and
// a release against both).  Releases are interleaved from inside the threads,
// so a lookup can meet an entry that was erased meanwhile (the dead-entry retry).
void check_threads() {
  constexpr int kThreads = 6, kStreams = 3, kCalls = 2000;
  static const size_t sizes[5] = {1, MiB, MiB + 1, 3 * MiB, 5 * MiB / 2};
  static long in_callback[kStreams];  // plain on purpose
  static long calls_done[kStreams];
  std::atomic<int> bad{0}, ready{0};
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([t, &bad, &ready] {
      const int si = t % kStreams;
      const hipStream_t s = fake_stream(0x10000 + 0x1000 * si);
      ++ready;
      while (ready < kThreads) std::this_thread::yield();
      for (int i = 0; i < kCalls; ++i) {
        // the first calls stay below 1 MiB: the two threads of a stream share
        // one buffer that nothing frees, ordered by the entry lock alone
        const size_t bytes = i < kCalls / 10 ? sizes[0] + 4096 * (i % 5) : sizes[(i + t) % 5];
        int runs = 0;
        const hipError_t e = qpb_with_workspace(s, bytes, [&](void *p) {
          ++runs;
          if (++in_callback[si] != 1) ++bad;
          if (live_bytes(p) < bytes) ++bad;
          else {
            unsigned char *c = static_cast<unsigned char *>(p);
            c[0] = (unsigned char)t;
            c[bytes - 1] = (unsigned char)i;
          }
          ++calls_done[si];
          --in_callback[si];
          return hipSuccess;
        });
        if (e != hipSuccess || runs != 1) ++bad;
        if (i < kCalls / 10) continue;
        if (i % 97 == 96 && qpb_release_stream_workspace(s) != 0) ++bad;
        if (i % 389 == 388 && qpb_release_workspaces() != 0) ++bad;
        if (i % 211 == 210 && qpb_release_stream_workspace(fake_stream(0x10000 + 0x1000 * ((si + 1) % kStreams))) != 0)
          ++bad;
      }
    });
  for (auto &x : th) x.join();
  CHECK(bad == 0);
  for (int s = 0; s < kStreams; ++s) CHECK(calls_done[s] == 2L * kCalls && in_callback[s] == 0);
  CHECK(live_count() <= (size_t)kStreams);
  CHECK(qpb_release_workspaces() == 0);
  CHECK(live_count() == 0);
  CHECK(g_mallocs == g_frees);
}
}  // namespace

int main() {
  check_identity();
  check_alloc_failure();
  check_threads();
  if (g_failures) {
    std::printf("ws_check FAILED: %d checks\n", g_failures);
    return 1;
  }
  std::printf("mallocs %ld frees %ld syncs %ld\nws_check ok\n", g_mallocs.load(), g_frees.load(), g_syncs.load());
  return 0;
}
