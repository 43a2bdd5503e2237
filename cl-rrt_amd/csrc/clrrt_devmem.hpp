// clrrt_devmem.hpp -- one owner for a context's device and pinned memory (no HIP include).
//
// Every long-lived buffer of a context is allocated, re-grown and freed through its DevMem: renew() is the one verb for
// members (allocate, or free the old block and allocate again), release() drops one, release_all() -- and the destructor
// -- whatever is still held, so no teardown lists any buffer and an allocation needs no far-away second edit.  The
// registry is keyed by pointer value, not by the member's address: swapped, rotated and copied structs of owned
// pointers need no care, and an alias into another block (WalkBufs::roster) is unknown to it and refused, never freed.
// Call-lifetime scratch is a DevScratch: unregistered, freed at scope exit, so entry points return early.
//
// Api binds the runtime: `err_t`, `ok`, `refused`, and static dev_alloc(void**, bytes), dev_free(void*),
// host_alloc(void**, bytes, flags), host_free(void*), and for the guard bands dev_fill(void*, byte, bytes) and
// copy_out(void* host_dst, const void* src, bytes) -- the latter waits for the device's queued work first and reads
// device or pinned memory (a policy may leave these two out: it then has no guard).  None of these calls belongs in a
// round: a device free
// synchronises the whole device.  A free's own result is dropped on purpose: the runtime fails one only with a sticky
// asynchronous error of earlier work, which the caller's next runtime call reports, and a block that could not be
// freed is forgotten all the same -- a teardown or a re-grow has no better use for it.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

namespace clrrt {

// Guard bands (a test facility; off, the product path, MemGuard hands out exactly the runtime's pointers).  With a
// guard of G bytes on -- a multiple of 256, so no block's alignment changes -- an allocation of n bytes takes n + 2 G
// from the runtime, both bands are filled with 0xFF (a stray read of one gives NaN or -1) and base + G is handed out.
// A block remembers its own G, so the guard may change between allocations.  The bands are checked when the block is
// freed and, for every live block, by check(); a violation found at a free is kept in the process-wide record (one per
// Api, i.e. per library) until the next check() reports it.  An overrun shorter than G stays inside memory the block
// owns: it is reported, and it damages no neighbour.
struct MemReport {
  int64_t blocks_checked = 0;       // live blocks, plus the blocks freed since the last check()
  int64_t guard_bytes_checked = 0;  // 2 G for each of them
  int64_t violations = 0;           // bands that no longer hold the pattern
  // the first of them (frees in their order, then live blocks by age): the block's allocation serial number (every
  // allocation of the process counts, guarded or not, from 1), its requested size, the band (-1: before the block, +1:
  // after it; 0: none) and the first changed byte's offset within the band
  int64_t first_serial = 0, first_bytes = 0, first_offset = 0;
  int32_t first_side = 0;
};

// Whether a policy has the guard's two verbs.  One without them (the four allocation verbs only) is still a policy of
// the owner: its guard stays off -- set() refuses anything but 0 -- and every pointer is the runtime's.
template <class Api, class = void>
struct has_guard_verbs : std::false_type {};
template <class Api>
struct has_guard_verbs<Api, std::void_t<decltype(Api::dev_fill((void*)nullptr, 0, size_t(0))),
                                        decltype(Api::copy_out((void*)nullptr, (const void*)nullptr, size_t(0)))>>
    : std::true_type {};

template <class Api>
class MemGuard {
 public:
  using err_t = typename Api::err_t;
  static constexpr size_t max_guard = size_t(1) << 20;
  static constexpr unsigned char pattern = 0xFF;
  static constexpr bool supported = has_guard_verbs<Api>::value;

  // The guard of the blocks allocated from now on: 0, or a multiple of 256 up to max_guard (else false).
  static bool set(size_t g) {
    if (g % 256 != 0 || g > max_guard || (g != 0 && !supported)) return false;
    state().guard.store(g);
    return true;
  }
  static size_t get() { return state().guard.load(); }

  // On failure *p is left as it was.
  static err_t alloc(void** p, size_t bytes, bool host, unsigned flags) {
    State& s = state();
    const int64_t serial = s.serial.fetch_add(1) + 1;
    const size_t g = s.guard.load();
    if (!g) return host ? Api::host_alloc(p, bytes, flags) : Api::dev_alloc(p, bytes);
    void* q = nullptr;
    err_t e = host ? Api::host_alloc(&q, bytes + 2 * g, flags) : Api::dev_alloc(&q, bytes + 2 * g);
    if (e != Api::ok || !q) return e != Api::ok ? e : Api::refused;
    char* base = (char*)q;
    if (host) {
      memset(base, pattern, g);
      memset(base + g + bytes, pattern, g);
    } else {
      e = fill(base, g);
      if (e == Api::ok) e = fill(base + g + bytes, g);
      if (e != Api::ok) {
        (void)Api::dev_free(q);
        return e;
      }
    }
    {
      std::lock_guard<std::mutex> lk(s.mu);
      s.live.push_back({base + g, serial, bytes, g, host});
      s.n_live.store(s.live.size());
    }
    *p = base + g;
    return Api::ok;
  }

  // Frees a pointer alloc() handed out (its bands checked first) or, unknown to the guard, passes it to the runtime.
  static err_t free(void* p, bool host) {
    State& s = state();
    size_t g = 0;
    if (s.n_live.load() != 0) {
      std::lock_guard<std::mutex> lk(s.mu);
      for (size_t i = 0; i < s.live.size(); i++)
        if (s.live[i].p == p) {
          check_block(s, s.live[i], s.freed);
          g = s.live[i].g;
          s.live.erase(s.live.begin() + (std::ptrdiff_t)i);
          s.n_live.store(s.live.size());
          break;
        }
    }
    void* base = (char*)p - g;
    return host ? Api::host_free(base) : Api::dev_free(base);
  }

  // Every live guarded block, and the record of the frees since the last call (which this clears).
  static void check(MemReport* out) {
    State& s = state();
    std::lock_guard<std::mutex> lk(s.mu);
    MemReport r = s.freed;
    s.freed = MemReport{};
    for (const Block& b : s.live) check_block(s, b, r);
    *out = r;
  }
  static size_t live() { return state().n_live.load(); }

 private:
  struct Block {
    void* p;  // as handed out
    int64_t serial;
    size_t bytes, g;
    bool host;
  };
  struct State {
    std::atomic<size_t> guard{0}, n_live{0};
    std::atomic<int64_t> serial{0};
    std::mutex mu;  // live, freed, tmp
    std::vector<Block> live;  // in allocation order
    MemReport freed;
    std::vector<unsigned char> tmp;
  };
  // (never destroyed: a context may be freed after the process's static destructors have begun)
  static State& state() {
    static State* s = new State;
    return *s;
  }
  // The policy's verbs (never reached for a policy without them: its guard is always 0 and no block is registered).
  static err_t fill(void* p, size_t n) {
    if constexpr (supported) return Api::dev_fill(p, pattern, n);
    else return Api::refused;
  }
  static err_t copy(void* dst, const void* src, size_t n) {
    if constexpr (supported) return Api::copy_out(dst, src, n);
    else return Api::refused;
  }
  // A block whose bands cannot be read (a sticky error of earlier work) is not counted as checked.
  static void check_block(State& s, const Block& b, MemReport& r) {
    s.tmp.resize(b.g);
    int64_t first[2] = {-1, -1};
    for (int side = 0; side < 2; side++) {
      const char* band = side ? (const char*)b.p + b.bytes : (const char*)b.p - b.g;
      if (copy(s.tmp.data(), band, b.g) != Api::ok) return;
      for (size_t k = 0; k < b.g && first[side] < 0; k++)
        if (s.tmp[k] != pattern) first[side] = (int64_t)k;
    }
    r.blocks_checked++;
    r.guard_bytes_checked += (int64_t)(2 * b.g);
    for (int side = 0; side < 2; side++) {
      if (first[side] < 0) continue;
      if (r.violations++ == 0) {
        r.first_serial = b.serial;
        r.first_bytes = (int64_t)b.bytes;
        r.first_offset = first[side];
        r.first_side = side ? 1 : -1;
      }
    }
  }
};

template <class Api>
class DevMem {
 public:
  using err_t = typename Api::err_t;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release_all(); }

  // *p null, or a block of this owner's (freed and forgotten first); then `count` elements (0: one).  On failure *p is
  // null and nothing is held for it.  A non-null *p this owner does not hold is refused and left alone.
  template <class T>
  err_t renew(T** p, size_t count) { return renew_as((void**)p, (count ? count : 1) * sizeof(T), false, 0); }
  err_t renew_bytes(void** p, size_t bytes) { return renew_as(p, bytes ? bytes : 1, false, 0); }
  template <class T>
  err_t renew_host(T** p, size_t count, unsigned flags = 0) {
    return renew_as((void**)p, (count ? count : 1) * sizeof(T), true, flags);
  }

  // Frees, forgets and nulls; null is a no-op (so is a second release); a pointer not held is refused and left alone.
  template <class T>
  err_t release(T** p) {
    if (!*p) return Api::ok;
    const size_t i = find(*p);
    if (i == held_.size()) return Api::refused;
    drop(i);
    *p = nullptr;
    return Api::ok;
  }

  void release_all() {
    while (!held_.empty()) drop(held_.size() - 1);
  }
  size_t held() const { return held_.size(); }

 private:
  struct Block {
    void* p;
    bool host;
  };
  std::vector<Block> held_;

  size_t find(const void* p) const {
    size_t i = 0;
    while (i < held_.size() && held_[i].p != p) i++;
    return i;
  }
  void drop(size_t i) {
    (void)MemGuard<Api>::free(held_[i].p, held_[i].host);
    held_[i] = held_.back();
    held_.pop_back();
  }
  err_t renew_as(void** p, size_t bytes, bool host, unsigned flags) {
    if (*p) {
      const size_t i = find(*p);
      if (i == held_.size() || held_[i].host != host) return Api::refused;  // an alias, or the other kind of memory
      drop(i);
      *p = nullptr;
    }
    held_.reserve(held_.size() + 1);  // before the allocation: a block is never made and then not held
    void* q = nullptr;
    const err_t e = MemGuard<Api>::alloc(&q, bytes, host, flags);
    if (e != Api::ok || !q) return e != Api::ok ? e : Api::refused;
    held_.push_back({q, host});
    *p = q;
    return Api::ok;
  }
};

// `count` elements of device scratch for one call: not registered, freed when it leaves scope.
template <class Api, class T>
class DevScratch {
 public:
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() {
    if (p) (void)MemGuard<Api>::free(p, false);
  }
  typename Api::err_t alloc(size_t count) {
    if (p) return Api::refused;
    return MemGuard<Api>::alloc((void**)&p, (count ? count : 1) * sizeof(T), false, 0);
  }
  operator T*() const { return p; }
  T* p = nullptr;
};

}  // namespace clrrt
