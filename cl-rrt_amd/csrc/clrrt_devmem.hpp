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
// host_alloc(void**, bytes, flags), host_free(void*).  None of these calls belongs in a round: a device free
// synchronises the whole device.  A free's own result is dropped on purpose: the runtime fails one only with a sticky
// asynchronous error of earlier work, which the caller's next runtime call reports, and a block that could not be
// freed is forgotten all the same -- a teardown or a re-grow has no better use for it.
#pragma once
#include <cstddef>
#include <vector>

namespace clrrt {

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
    if (held_[i].host) (void)Api::host_free(held_[i].p);
    else (void)Api::dev_free(held_[i].p);
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
    const err_t e = host ? Api::host_alloc(&q, bytes, flags) : Api::dev_alloc(&q, bytes);
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
    if (p) (void)Api::dev_free(p);
  }
  typename Api::err_t alloc(size_t count) {
    if (p) return Api::refused;
    return Api::dev_alloc((void**)&p, (count ? count : 1) * sizeof(T));
  }
  operator T*() const { return p; }
  T* p = nullptr;
};

}  // namespace clrrt
