// cmpc_host_buffers.h — private to cmpc_abi.cpp: the owner of one runtime allocation and the layout
// of the single-instance staging. No HIP in here, so both compile (and are checked) on the host
// alone; cmpc_abi.cpp supplies the two allocators (hipMalloc / hipFree, hipHostMalloc / hipHostFree).
#pragma once

#include <cstddef>
#include <utility>

#include "../../include/cmpc_solver.h"

namespace cmpc {

// Move-only owner of one allocation of T[count], released by reset() or the destructor. A states
// how: A::alloc(void** p, size_t bytes, flags...) returns the runtime's error code (0: success) and
// A::release(void* p) frees. A failed alloc() leaves the owner empty, so a ladder of them unwinds
// by leaving scope and a later call can try again.
template <class T, class A>
class Owned {
 public:
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  ~Owned() { reset(); }

  template <class... Flags>
  auto alloc(size_t count, Flags... flags) {
    reset();
    void* p = nullptr;
    const auto e = A::alloc(&p, count * sizeof(T), flags...);
    if (e == 0) p_ = static_cast<T*>(p);
    return e;
  }
  void reset() {
    if (p_) A::release(p_);
    p_ = nullptr;
  }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
};

// Staging of the single-instance round trip (cmpc_abi.cpp single_round_trip), in floats, sized for
// the largest horizon. In, pinned and on the device (d_rec, behind its last record): the record,
// then up to kPad words (the reference surface's f_ext[3] and simulation_time). Out, pinned and on
// the device (d_single_out): the forces [12 N], the status word, then up to kPad - 1 words (f_est(3)).
struct SingleStage {
  static constexpr size_t kPad = 4;
  static constexpr size_t kRecMax = CMPC_REC_WORDS(CMPC_MAX_HORIZON);
  static constexpr size_t kForcesMax = 12 * (size_t)CMPC_MAX_HORIZON;
  static constexpr size_t kInWords = kRecMax + kPad;        // (d_rec: max_batch records + kPad)
  static constexpr size_t kOutWords = kForcesMax + kPad;    // d_single_out
  static constexpr size_t kPinOut = kInWords;               // the pinned buffer: in, then out
  static constexpr size_t kPinWords = kInWords + kOutWords;
  static constexpr size_t status_word(int N) { return 12 * (size_t)N; }
  static constexpr size_t out_words(int N, int extra) { return status_word(N) + 1 + (size_t)extra; }
};
static_assert(SingleStage::out_words(CMPC_MAX_HORIZON, SingleStage::kPad - 1) <= SingleStage::kOutWords,
              "single-instance staging: the words behind the status word do not fit");

}  // namespace cmpc
