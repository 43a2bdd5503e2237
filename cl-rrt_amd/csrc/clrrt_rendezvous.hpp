// clrrt_rendezvous.hpp — the host meeting point of the in-process exchange transport (include/clrrt_xchg.h): the ranks
// of one process, one thread each, meet twice per exchange.  Host C++ only (no HIP), so a host program can test it on
// its own (tests/native/rendezvous_check.cpp, under -fsanitize=thread).
//
// meet() is a reusable barrier with a deadline: it returns true once all `world` threads of the current generation
// have arrived, and false when the deadline passed first or the rendezvous was broken.  A timeout breaks the
// rendezvous for good -- every waiter and every later caller gets false at once -- so no rank ever waits forever for
// a peer that left.  What a thread wrote before meet() is visible to every thread after their meet() of the same
// generation returned true (the barrier's mutex orders them).
#ifndef CLRRT_RENDEZVOUS_HPP
#define CLRRT_RENDEZVOUS_HPP

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>

namespace clrrt_xchg_detail {

class Rendezvous {
 public:
  Rendezvous(int world, int timeout_ms) : world_(world), timeout_(timeout_ms) {}
  Rendezvous(const Rendezvous&) = delete;
  Rendezvous& operator=(const Rendezvous&) = delete;

  bool meet() {
    std::unique_lock<std::mutex> lk(m_);
    if (broken_) return false;
    const uint64_t gen = gen_;
    if (++arrived_ == world_) {
      arrived_ = 0;
      gen_++;
      cv_.notify_all();
      return true;
    }
    // (system_clock: its timed wait is the plain pthread_cond_timedwait every thread sanitizer knows)
    const auto deadline = std::chrono::system_clock::now() + timeout_;
    while (gen_ == gen && !broken_) {
      if (cv_.wait_until(lk, deadline) == std::cv_status::timeout && gen_ == gen && !broken_) {
        broken_ = true;
        cv_.notify_all();
      }
    }
    return gen_ != gen;
  }
  // A rank that cannot go on (an error between two meetings) releases its peers at once instead of at the deadline.
  void abandon() {
    std::lock_guard<std::mutex> lk(m_);
    broken_ = true;
    cv_.notify_all();
  }
  bool broken() {
    std::lock_guard<std::mutex> lk(m_);
    return broken_;
  }
  int world() const { return world_; }
  // completed meetings (tests)
  uint64_t generation() {
    std::lock_guard<std::mutex> lk(m_);
    return gen_;
  }

 private:
  const int world_;
  const std::chrono::milliseconds timeout_;
  std::mutex m_;
  std::condition_variable cv_;
  int arrived_ = 0;
  uint64_t gen_ = 0;
  bool broken_ = false;
};

}  // namespace clrrt_xchg_detail

#endif  // CLRRT_RENDEZVOUS_HPP
