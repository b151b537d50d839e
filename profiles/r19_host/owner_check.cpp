// Host-only check of csrc/cmpc_host_buffers.h: the buffer owner under a stubbed allocator and the
// single-instance staging layout. No GPU, no HIP, no Python.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined profiles/r19_host/owner_check.cpp -o owner_check
// (or the same with g++ / clang++ and plain -fsanitize=...). Exit status 0 and "owner_check: ok"
// with no sanitizer report: no leak, no double free, no use after free, no overrun.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../../quad-periodic-mpc_amd/csrc/cmpc_host_buffers.h"

namespace {
int g_live = 0;        // allocations not yet released
int g_allocs = 0;      // alloc() calls that succeeded
int g_fail_at = -1;    // the alloc() call (0-based, counted from arm()) that fails; -1: none
int g_calls = 0;
unsigned g_last_flags = 0;

void arm(int fail_at) {
  g_fail_at = fail_at;
  g_calls = 0;
}

// the runtime's shape: an error code (0: success), memory from malloc so the sanitizer sees it
struct StubAlloc {
  static int alloc(void** p, size_t bytes, unsigned flags = 0) {
    g_last_flags = flags;
    if (g_calls++ == g_fail_at) return 2;  // (hipErrorOutOfMemory's value)
    *p = std::malloc(bytes ? bytes : 1);
    if (!*p) return 2;
    g_live++;
    g_allocs++;
    return 0;
  }
  static void release(void* p) {
    g_live--;
    std::free(p);
  }
};
template <class T> using Buf = cmpc::Owned<T, StubAlloc>;

int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      g_failed++;                                                        \
    }                                                                    \
  } while (0)

// three allocations, all or nothing, as ensure_inst_buffers takes them
struct Three {
  Buf<double> a;
  Buf<float> b;
  Buf<int> c;
};
int ensure_three(Three& t, size_t n) {
  if (t.a) return 0;
  Buf<double> a;
  Buf<float> b;
  Buf<int> c;
  int e;
  if ((e = a.alloc(6 * n)) != 0 || (e = b.alloc(n)) != 0 || (e = c.alloc(1)) != 0) return e;
  t.a = std::move(a);
  t.b = std::move(b);
  t.c = std::move(c);
  return 0;
}

// allocations into the members themselves, reset on failure, as ensure_staging takes them
struct Staged {
  Buf<float> rec, out;
  Buf<float> pin;
  bool staged = false;
  void free_all() {
    rec.reset();
    out.reset();
    pin.reset();
    staged = false;
  }
};
int ensure_staged(Staged& s, size_t batch) {
  if (s.staged) return 0;
  using St = cmpc::SingleStage;
  int e;
  if ((e = s.rec.alloc(St::kRecMax * batch + St::kPad)) == 0 && (e = s.out.alloc(St::kOutWords)) == 0 &&
      (e = s.pin.alloc(St::kPinWords, 1u)) == 0) {
    s.staged = true;
    return 0;
  }
  s.free_all();
  return e;
}
}  // namespace

int main() {
  arm(-1);
  {  // alloc, get, write the whole extent, release by the destructor
    Buf<float> a;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.alloc(100) == 0 && a && g_live == 1);
    std::memset(a.get(), 0x5a, 100 * sizeof(float));
  }
  CHECK(g_live == 0);
  {  // reset, double reset, reset of an empty owner
    Buf<int> a, b;
    CHECK(a.alloc(8) == 0);
    a.reset();
    CHECK(!a && g_live == 0);
    a.reset();
    b.reset();
    CHECK(g_live == 0);
  }
  {  // move construction and move assignment: one owner at a time, the target's old buffer released
    Buf<double> a;
    CHECK(a.alloc(4) == 0);
    double* p = a.get();
    Buf<double> b(std::move(a));
    CHECK(!a && b.get() == p && g_live == 1);
    Buf<double> c;
    CHECK(c.alloc(4) == 0 && g_live == 2);
    c = std::move(b);
    CHECK(!b && c.get() == p && g_live == 1);
    Buf<double>& self = c;
    c = std::move(self);  // self-assignment keeps the buffer
    CHECK(c.get() == p && g_live == 1);
    c.get()[3] = 1.0;
  }
  CHECK(g_live == 0);
  {  // a second alloc releases the first; a failed alloc leaves the owner empty and a later one works
    Buf<float> a;
    CHECK(a.alloc(4) == 0 && a.alloc(16) == 0 && g_live == 1);
    arm(0);
    CHECK(a.alloc(32) == 2 && !a && g_live == 0);
    arm(-1);
    CHECK(a.alloc(32) == 0 && a && g_live == 1);
    a.get()[31] = 1.f;
  }
  CHECK(g_live == 0);
  {  // flags reach the allocator; none given: its default
    Buf<int> a;
    CHECK(a.alloc(4, 7u) == 0 && g_last_flags == 7u);
    CHECK(a.alloc(4) == 0 && g_last_flags == 0u);
  }
  // the ladder of locals: whichever step fails, nothing is kept and nothing leaks; then a retry succeeds
  for (int fail_at = 0; fail_at < 3; fail_at++) {
    Three t;
    arm(fail_at);
    CHECK(ensure_three(t, 5) == 2 && !t.a && !t.b && !t.c && g_live == 0);
    arm(-1);
    CHECK(ensure_three(t, 5) == 0 && t.a && t.b && t.c && g_live == 3);
    const int before = g_allocs;
    CHECK(ensure_three(t, 5) == 0 && g_allocs == before);  // (already there: no allocation)
  }
  CHECK(g_live == 0);
  // the ladder into the members: all or nothing, and a later call tries again
  for (int fail_at = 0; fail_at < 3; fail_at++) {
    Staged s;
    arm(fail_at);
    CHECK(ensure_staged(s, 3) == 2 && !s.staged && !s.rec && !s.out && !s.pin && g_live == 0);
    arm(-1);
    CHECK(ensure_staged(s, 3) == 0 && s.staged && g_live == 3 && g_last_flags == 1u);
    // the round trip's extents, at the largest horizon and with every extra word, lie inside
    using St = cmpc::SingleStage;
    const int N = CMPC_MAX_HORIZON;
    float* pin = s.pin.get();
    std::memset(pin, 0, (CMPC_REC_WORDS(N) + 2) * sizeof(float));                // record + 2 words in
    std::memset(pin + St::kPinOut, 0, St::out_words(N, 1) * sizeof(float));      // forces, status, f_est(3)
    std::memset(s.rec.get(), 0, (CMPC_REC_WORDS(N) + 2) * sizeof(float));
    std::memset(s.out.get(), 0, St::out_words(N, 1) * sizeof(float));
    s.free_all();
    s.free_all();
    CHECK(g_live == 0);
  }
  // the layout is the one the literals stated
  using St = cmpc::SingleStage;
  static_assert(St::kPinOut == CMPC_REC_WORDS(CMPC_MAX_HORIZON) + 4, "pinned out area");
  static_assert(St::kPinWords == CMPC_REC_WORDS(CMPC_MAX_HORIZON) + 4 + 12 * CMPC_MAX_HORIZON + 4, "pinned words");
  static_assert(St::kOutWords == 12 * CMPC_MAX_HORIZON + 4, "d_single_out");
  static_assert(St::out_words(10, 0) == 12 * 10 + 1 && St::out_words(10, 1) == 12 * 10 + 2, "D2H words");
  static_assert(St::status_word(16) == 12 * 16, "status word");
  CHECK(g_live == 0);
  if (g_failed) return 1;
  std::printf("owner_check: ok (%d allocations, %d live at exit)\n", g_allocs, g_live);
  return 0;
}
