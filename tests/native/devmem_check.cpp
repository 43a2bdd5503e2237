// devmem_check.cpp -- the context's memory owner (cl-rrt_amd/csrc/clrrt_devmem.hpp, no HIP) on the host: a policy of
// counting malloc / free fakes with a "fail the k-th allocation" switch.  Built with -fsanitize=address,undefined by
// tests/test_devmem_host.py: the counters are the "freed exactly once" oracle, the sanitizer's leak check at exit the
// "nothing leaked" one.  The guard bands (clrrt::MemGuard) are checked here too: a byte planted at either end of either
// band -- inside the fake's malloc block, so the sanitizer has nothing to say -- must be reported with its side and
// offset, by a check of the live blocks and at a free.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "../../cl-rrt_amd/csrc/clrrt_devmem.hpp"

static int g_fail = 0;

struct Fake {
  using err_t = int;
  static constexpr int ok = 0, refused = 1, nomem = 2;
  static inline long n_alloc = 0, n_dev_alloc = 0, n_dev_free = 0, n_host_alloc = 0, n_host_free = 0, crossed = 0;
  static inline long fail_at = 0;  // the k-th allocation from now fails (0: none)
  static inline std::set<void*> dev, host;
  static int alloc(void** p, size_t bytes, std::set<void*>& live, long& n) {
    if (fail_at > 0 && --fail_at == 0) return nomem;
    *p = malloc(bytes);
    live.insert(*p);
    n++;
    n_alloc++;
    return ok;
  }
  static int free_(void* p, std::set<void*>& live, long& n) {
    if (!live.erase(p)) {  // the other side's pointer, a foreign one or a second free: never passed on to free()
      crossed++;
      return refused;
    }
    free(p);
    n++;
    return ok;
  }
  static int dev_alloc(void** p, size_t bytes) { return alloc(p, bytes, dev, n_dev_alloc); }
  static int dev_free(void* p) { return free_(p, dev, n_dev_free); }
  static int host_alloc(void** p, size_t bytes, unsigned) { return alloc(p, bytes, host, n_host_alloc); }
  static int host_free(void* p) { return free_(p, host, n_host_free); }
  static inline long n_fill = 0, n_copy = 0;
  static int dev_fill(void* p, int byte, size_t bytes) {
    memset(p, byte, bytes);
    n_fill++;
    return ok;
  }
  static int copy_out(void* dst, const void* src, size_t bytes) {
    memcpy(dst, src, bytes);
    n_copy++;
    return ok;
  }
  static void reset() {
    n_alloc = n_dev_alloc = n_dev_free = n_host_alloc = n_host_free = crossed = fail_at = 0;
  }
  static bool balanced() {
    return dev.empty() && host.empty() && n_dev_alloc == n_dev_free && n_host_alloc == n_host_free && crossed == 0;
  }
};
using Mem = clrrt::DevMem<Fake>;
using Guard = clrrt::MemGuard<Fake>;
// the runtime's pointer of a block handed out under the current guard
static void* raw(void* p) { return (char*)p - Guard::get(); }

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      g_fail++;                                                  \
    }                                                            \
  } while (0)

// A buffer set shaped like WalkBufs: 28 members, a byte-sized one and an alias among them, `P` allocated last.
struct Set {
  int* m[26] = {};
  void* tmp = nullptr;
  int* roster = nullptr;  // alias into m[3]
  int* P = nullptr;
};
static int alloc_set(Mem& mem, Set& w) {
  if (w.P) return Fake::ok;
  int e;
  for (int i = 0; i < 26; i++)
    if ((e = mem.renew(&w.m[i], 8 + i)) != Fake::ok) return e;
  w.roster = w.m[3] + 2;
  if ((e = mem.renew_bytes(&w.tmp, 256)) != Fake::ok) return e;
  return mem.renew(&w.P, 16);  // last: marks the set complete
}

static void t_renew_frees_once() {
  Fake::reset();
  {
    Mem mem;
    int* p = nullptr;
    CHECK(mem.renew(&p, 4) == Fake::ok && p && mem.held() == 1);
    int* old = p;
    CHECK(mem.renew(&p, 8) == Fake::ok && p && mem.held() == 1);
    CHECK(Fake::n_dev_alloc == 2 && Fake::n_dev_free == 1 && !Fake::dev.count(old));
    double* z = nullptr;
    CHECK(mem.renew(&z, 0) == Fake::ok && z);  // a count of 0 allocates one element
    z[0] = 1.0;
  }
  CHECK(Fake::n_dev_free == 3 && Fake::balanced());
}

static void t_fail_every_k() {
  for (long k = 1; k <= 28; k++) {
    Fake::reset();
    {
      Mem mem;
      Set w;
      Fake::fail_at = k;
      CHECK(alloc_set(mem, w) == Fake::nomem);
      CHECK(!w.P && mem.held() == (size_t)(k - 1));
      if (k <= 26) CHECK(w.m[k - 1] == nullptr);
      if (k == 27) CHECK(w.tmp == nullptr);
      const long before = Fake::n_dev_free;
      CHECK(alloc_set(mem, w) == Fake::ok && w.P);  // the retry renews the earlier members, losing none
      CHECK(Fake::n_dev_free - before == k - 1 && mem.held() == 28);
      CHECK(alloc_set(mem, w) == Fake::ok && Fake::n_dev_alloc == 28 + (k - 1));  // complete: nothing more
    }
    CHECK(Fake::balanced());
  }
  // a failed renew over a live pointer: the old block is gone, the pointer null, nothing held for it
  Fake::reset();
  {
    Mem mem;
    int* p = nullptr;
    CHECK(mem.renew(&p, 4) == Fake::ok);
    Fake::fail_at = 1;
    CHECK(mem.renew(&p, 8) == Fake::nomem && !p && mem.held() == 0 && Fake::n_dev_free == 1);
    CHECK(mem.renew(&p, 8) == Fake::ok && p);
  }
  CHECK(Fake::balanced());
}

static void t_release_and_foreign() {
  Fake::reset();
  int outside[4] = {};
  {
    Mem mem;
    int *p = nullptr, *keep = nullptr;
    CHECK(mem.renew(&p, 4) == Fake::ok && mem.renew(&keep, 4) == Fake::ok);
    int* copy = p;
    CHECK(mem.release(&p) == Fake::ok && !p && Fake::n_dev_free == 1);
    CHECK(mem.release(&p) == Fake::ok && Fake::n_dev_free == 1);           // null: a no-op
    CHECK(mem.release(&copy) == Fake::refused && Fake::n_dev_free == 1);  // already forgotten: never freed twice
    // a foreign pointer and an alias into an owned block: refused, left alone, never freed
    int* f = outside;
    CHECK(mem.renew(&f, 4) == Fake::refused && f == outside);
    CHECK(mem.release(&f) == Fake::refused && f == outside);
    int* alias = keep + 1;
    CHECK(mem.renew(&alias, 4) == Fake::refused && alias == keep + 1);
    void* bytes = nullptr;
    CHECK(mem.renew_bytes(&bytes, 0) == Fake::ok && bytes);
    CHECK(mem.release(&bytes) == Fake::ok && !bytes);
    CHECK(Fake::n_dev_alloc == 3 && Fake::n_dev_free == 2 && Fake::crossed == 0);
  }
  CHECK(Fake::balanced());
}

static void t_swap_structs() {
  Fake::reset();
  {
    Mem mem;
    Set a, b, lag[3];
    CHECK(alloc_set(mem, a) == Fake::ok && alloc_set(mem, b) == Fake::ok);
    std::swap(a, b);
    Set copy = a;  // a struct copy, as the drivers take of their slots
    for (Set& s : lag) CHECK(alloc_set(mem, s) == Fake::ok);
    std::swap(lag[0], lag[2]);
    std::swap(lag[0], lag[1]);  // a rotation
    CHECK(mem.renew(&copy.m[0], 64) == Fake::ok);  // renewing through the copy frees the shared block once
    a.m[0] = copy.m[0];
    CHECK(mem.held() == 5 * 28);
    mem.release_all();
    CHECK(mem.held() == 0 && Fake::n_dev_alloc == 5 * 28 + 1 && Fake::n_dev_free == Fake::n_dev_alloc);
    mem.release_all();  // and the destructor after it: nothing more
  }
  CHECK(Fake::balanced());
}

static int scratch_exit(int leave_at) {
  clrrt::DevScratch<Fake, double> a, b;
  clrrt::DevScratch<Fake, char> unused;
  if (a.alloc(10) != Fake::ok) return 1;
  if (leave_at == 1) return 2;
  if (b.alloc(0) != Fake::ok) return 3;
  a[9] = b[0] = 1.0;
  if (a.alloc(4) != Fake::refused) return 4;  // one allocation per scratch
  if (leave_at == 2) return 5;
  return 0;
}
static void t_scratch() {
  for (int leave = 0; leave <= 2; leave++)
    for (long k = 0; k <= 2; k++) {
      Fake::reset();
      Fake::fail_at = k;
      const int rc = scratch_exit(leave);
      CHECK(rc == (k == 1 ? 1 : leave == 1 ? 2 : k == 2 ? 3 : leave == 2 ? 5 : 0));
      CHECK(Fake::balanced());
    }
}

static void t_sides_never_cross() {
  Fake::reset();
  {
    Mem mem;
    int *d = nullptr, *h = nullptr;
    CHECK(mem.renew(&d, 4) == Fake::ok && mem.renew_host(&h, 4, 2u) == Fake::ok);
    CHECK(Fake::dev.count(raw(d)) && Fake::host.count(raw(h)));
    int *d0 = d, *h0 = h;
    CHECK(mem.renew_host(&d, 4) == Fake::refused && d == d0);  // a device block is not renewed as pinned memory
    CHECK(mem.renew(&h, 4) == Fake::refused && h == h0);
    CHECK(mem.renew_host(&h, 8) == Fake::ok && Fake::n_host_free == 1 && Fake::n_dev_free == 0);
    std::swap(d, h);  // whatever member holds it, a block goes back to the side it came from
    CHECK(mem.release(&d) == Fake::ok && Fake::n_host_free == 2 && Fake::n_dev_free == 0);
  }
  CHECK(Fake::n_dev_free == 1 && Fake::crossed == 0 && Fake::balanced());
}

// ---------------------------------------------------------------------------------------------- guard bands
static clrrt::MemReport report() {
  clrrt::MemReport r;
  Guard::check(&r);
  return r;
}
static bool clean(const clrrt::MemReport& r, long blocks, size_t G) {
  return r.blocks_checked == blocks && r.guard_bytes_checked == (int64_t)(2 * G) * blocks && r.violations == 0 &&
         r.first_side == 0;
}

static void t_guard_values() {
  CHECK(Guard::get() == 0);
  for (size_t bad : {(size_t)1, (size_t)255, (size_t)257, (size_t)1000, ((size_t)1 << 20) + 256, (size_t)1 << 21})
    CHECK(!Guard::set(bad) && Guard::get() == 0);
  for (size_t good : {(size_t)256, (size_t)65536, (size_t)1 << 20, (size_t)0}) CHECK(Guard::set(good) && Guard::get() == good);
}

// G = 0: exactly the runtime's pointers, no fill, no copy, nothing registered.
static void t_guard_off_passes_through() {
  Fake::reset();
  Fake::n_fill = Fake::n_copy = 0;
  {
    Mem mem;
    int *d = nullptr, *h = nullptr;
    CHECK(mem.renew(&d, 4) == Fake::ok && mem.renew_host(&h, 4) == Fake::ok);
    CHECK(Fake::dev.count(d) && Fake::host.count(h) && Guard::live() == 0);
    clrrt::DevScratch<Fake, int> s;
    CHECK(s.alloc(3) == Fake::ok && Fake::dev.count(s.p));
    CHECK(clean(report(), 0, 0));
  }
  CHECK(Fake::n_fill == 0 && Fake::n_copy == 0 && Fake::balanced() && clean(report(), 0, 0));
}

// The band bytes a test plants: (side, offset) = the first and last byte of each band.
struct Spot {
  int side;
  size_t off;
};
static unsigned char* spot(void* p, size_t bytes, size_t G, Spot s) {
  return (unsigned char*)p + (s.side < 0 ? -(std::ptrdiff_t)G : (std::ptrdiff_t)bytes) + (std::ptrdiff_t)s.off;
}
static bool names(const clrrt::MemReport& r, int64_t serial, size_t bytes, Spot s) {
  return r.violations == 1 && (serial < 0 || r.first_serial == serial) && r.first_bytes == (int64_t)bytes &&
         r.first_side == s.side && r.first_offset == (int64_t)s.off;
}

static void t_guard_reports(size_t G) {
  const Spot spots[4] = {{-1, 0}, {-1, G - 1}, {+1, 0}, {+1, G - 1}};
  Fake::reset();
  CHECK(Guard::set(G));
  for (int kind = 0; kind < 3; kind++) {  // a device block, a pinned block, a scratch block
    for (const Spot sp : spots) {
      for (int at_free = 0; at_free < 2; at_free++) {
        Mem mem;
        clrrt::DevScratch<Fake, char>* sc = new clrrt::DevScratch<Fake, char>;
        char *before = nullptr, *blk = nullptr, *after = nullptr;
        const size_t bytes = 37;  // no multiple of anything: the trailing band starts at an odd address
        CHECK(mem.renew(&before, 5) == Fake::ok);
        if (kind == 0) CHECK(mem.renew(&blk, bytes) == Fake::ok);
        if (kind == 1) CHECK(mem.renew_host(&blk, bytes) == Fake::ok);
        if (kind == 2) CHECK(sc->alloc(bytes) == Fake::ok && (blk = sc->p));
        CHECK(mem.renew(&after, 5) == Fake::ok);
        CHECK(blk && (kind == 1 ? Fake::host : Fake::dev).count(blk - G) && Guard::live() == 3);
        // the bands hold the pattern, the block between them is the caller's
        bool filled = true;
        for (size_t k = 0; k < G; k++) filled = filled && (unsigned char)blk[k - G] == 0xFF && (unsigned char)blk[bytes + k] == 0xFF;
        CHECK(filled);
        memset(blk, 0, bytes);
        CHECK(clean(report(), 3, G));
        // serial numbers count allocations: `blk` is one after `before`
        *spot(before, 5, G, {+1, 3}) = 0;
        clrrt::MemReport r = report();
        CHECK(names(r, -1, 5, {+1, 3}));
        const int64_t serial = r.first_serial + 1;
        *spot(before, 5, G, {+1, 3}) = 0xFF;
        CHECK(clean(report(), 3, G));
        *spot(blk, bytes, G, sp) = 0xFE;  // one changed bit
        if (!at_free) {
          r = report();
          CHECK(r.blocks_checked == 3 && names(r, serial, bytes, sp));
          r = report();  // still there: a live block is reported by every check
          CHECK(r.blocks_checked == 3 && names(r, serial, bytes, sp));
          *spot(blk, bytes, G, sp) = 0xFF;
          CHECK(clean(report(), 3, G));
          delete sc;
          mem.release_all();
          CHECK(clean(report(), 3, G));  // the three frees, nothing live
        } else {
          if (kind == 2) delete sc;
          else CHECK(mem.release(&blk) == Fake::ok);
          CHECK(Guard::live() == 2);
          r = report();  // the free's finding and the two live blocks
          CHECK(r.blocks_checked == 3 && r.guard_bytes_checked == (int64_t)(6 * G) && names(r, serial, bytes, sp));
          CHECK(clean(report(), 2, G));  // reported once
          if (kind != 2) delete sc;
          mem.release_all();
          CHECK(clean(report(), 2, G));  // the two remaining frees, nothing live
        }
      }
    }
  }
  CHECK(Guard::live() == 0 && Fake::balanced() && Fake::n_dev_alloc > 0 && Fake::n_host_alloc > 0);
  // two blocks changed: both counted, the older one named; a re-grow is a free
  {
    Mem mem;
    int *a = nullptr, *b = nullptr;
    CHECK(mem.renew(&a, 3) == Fake::ok && mem.renew(&b, 9) == Fake::ok);
    *spot(b, 36, G, {-1, 7}) = 1;
    *spot(b, 36, G, {+1, 0}) = 1;
    *spot(a, 12, G, {+1, 1}) = 1;
    clrrt::MemReport r = report();
    CHECK(r.violations == 3 && r.first_bytes == 12 && r.first_side == 1 && r.first_offset == 1);
    CHECK(mem.renew(&b, 20) == Fake::ok);  // b's two bands are found at this free, a's by the check of live blocks
    r = report();
    CHECK(r.blocks_checked == 3 && r.violations == 3 && r.first_bytes == 36 && r.first_side == -1 && r.first_offset == 7);
    *spot(a, 12, G, {+1, 1}) = 0xFF;
    CHECK(clean(report(), 2, G));
  }
  CHECK(clean(report(), 2, G) && Fake::balanced());
  // a failed allocation under the guard: the pointer stays null, nothing registered
  {
    Mem mem;
    int* p = nullptr;
    Fake::fail_at = 1;
    CHECK(mem.renew(&p, 4) == Fake::nomem && !p && Guard::live() == 0 && mem.held() == 0);
    clrrt::DevScratch<Fake, int> s;
    Fake::fail_at = 1;
    CHECK(s.alloc(4) == Fake::nomem && !s.p && Guard::live() == 0);
  }
  CHECK(Guard::set(0) && clean(report(), 0, 0) && Fake::balanced());
}

// Blocks remember their own guard: allocated under one G, checked and freed under another.
static void t_guard_switched() {
  Fake::reset();
  const size_t Gs[3] = {0, 256, 1024};
  for (size_t g_alloc : Gs)
    for (size_t g_free : Gs) {
      Mem mem;
      char *d = nullptr, *h = nullptr;
      CHECK(Guard::set(g_alloc));
      clrrt::DevScratch<Fake, char>* sc = new clrrt::DevScratch<Fake, char>;
      CHECK(mem.renew(&d, 100) == Fake::ok && mem.renew_host(&h, 100) == Fake::ok && sc->alloc(100) == Fake::ok);
      CHECK(Fake::dev.count(d - g_alloc) && Fake::host.count(h - g_alloc) && Fake::dev.count(sc->p - g_alloc));
      CHECK(Guard::set(g_free));
      char* d2 = nullptr;
      CHECK(mem.renew(&d2, 50) == Fake::ok && Fake::dev.count(d2 - g_free));
      const long live = (g_alloc ? 3 : 0) + (g_free ? 1 : 0);
      clrrt::MemReport r = report();
      CHECK(r.blocks_checked == live && r.guard_bytes_checked == (int64_t)(6 * g_alloc + 2 * g_free) && r.violations == 0);
      if (g_alloc) {  // found at the free, with the band length the block was allocated with
        *spot(h, 100, g_alloc, {+1, g_alloc - 1}) = 0;
        CHECK(mem.release(&h) == Fake::ok);
        r = report();
        CHECK(names(r, -1, 100, {+1, g_alloc - 1}));
      }
      delete sc;
      mem.release_all();
      r = report();
      CHECK(r.violations == 0 && Guard::live() == 0);
      CHECK(Fake::balanced());  // every runtime pointer went back as it came: none refused by the fake
    }
  CHECK(Guard::set(0));
}

// A policy with the four allocation verbs only is still the owner's: it has no guard, and every pointer is its own.
struct Bare {
  using err_t = int;
  static constexpr int ok = 0, refused = 1;
  static inline long live = 0;
  static int dev_alloc(void** p, size_t bytes) { return *p = malloc(bytes), live++, ok; }
  static int dev_free(void* p) { return free(p), live--, ok; }
  static int host_alloc(void** p, size_t bytes, unsigned) { return dev_alloc(p, bytes); }
  static int host_free(void* p) { return dev_free(p); }
};
static void t_policy_without_the_verbs() {
  using BG = clrrt::MemGuard<Bare>;
  static_assert(!BG::supported && Guard::supported, "verb detection");
  CHECK(!BG::set(256) && BG::get() == 0 && BG::set(0));
  {
    clrrt::DevMem<Bare> mem;
    int *d = nullptr, *h = nullptr;
    CHECK(mem.renew(&d, 4) == Bare::ok && mem.renew_host(&h, 4) == Bare::ok && mem.renew(&d, 9) == Bare::ok);
    d[8] = h[3] = 1;
    clrrt::DevScratch<Bare, double> s;
    CHECK(s.alloc(2) == Bare::ok && Bare::live == 3 && BG::live() == 0);
    clrrt::MemReport r;
    BG::check(&r);
    CHECK(r.blocks_checked == 0 && r.violations == 0);
  }
  CHECK(Bare::live == 0);
}

int main() {
  t_policy_without_the_verbs();
  t_guard_values();
  t_guard_off_passes_through();
  for (size_t G : {(size_t)0, (size_t)256}) {  // the owner's own checks, without the guard and under it
    CHECK(Guard::set(G));
    t_renew_frees_once();
    t_fail_every_k();
    t_release_and_foreign();
    t_swap_structs();
    t_scratch();
    t_sides_never_cross();
    CHECK(report().violations == 0 && Guard::live() == 0);
  }
  CHECK(Guard::set(0));
  t_guard_reports(256);
  t_guard_reports(65536);
  t_guard_switched();
  printf("devmem_check: failures %d\n", g_fail);
  return g_fail ? 1 : 0;
}
