// devmem_check.cpp -- the context's memory owner (cl-rrt_amd/csrc/clrrt_devmem.hpp, no HIP) on the host: a policy of
// counting malloc / free fakes with a "fail the k-th allocation" switch.  Built with -fsanitize=address,undefined by
// tests/test_devmem_host.py: the counters are the "freed exactly once" oracle, the sanitizer's leak check at exit the
// "nothing leaked" one.
#include <cstdio>
#include <cstdlib>
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
  static void reset() {
    n_alloc = n_dev_alloc = n_dev_free = n_host_alloc = n_host_free = crossed = fail_at = 0;
  }
  static bool balanced() {
    return dev.empty() && host.empty() && n_dev_alloc == n_dev_free && n_host_alloc == n_host_free && crossed == 0;
  }
};
using Mem = clrrt::DevMem<Fake>;

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
    CHECK(Fake::dev.count(d) && Fake::host.count(h));
    int *d0 = d, *h0 = h;
    CHECK(mem.renew_host(&d, 4) == Fake::refused && d == d0);  // a device block is not renewed as pinned memory
    CHECK(mem.renew(&h, 4) == Fake::refused && h == h0);
    CHECK(mem.renew_host(&h, 8) == Fake::ok && Fake::n_host_free == 1 && Fake::n_dev_free == 0);
    std::swap(d, h);  // whatever member holds it, a block goes back to the side it came from
    CHECK(mem.release(&d) == Fake::ok && Fake::n_host_free == 2 && Fake::n_dev_free == 0);
  }
  CHECK(Fake::n_dev_free == 1 && Fake::crossed == 0 && Fake::balanced());
}

int main() {
  t_renew_frees_once();
  t_fail_every_k();
  t_release_and_foreign();
  t_swap_structs();
  t_scratch();
  t_sides_never_cross();
  printf("devmem_check: failures %d\n", g_fail);
  return g_fail ? 1 : 0;
}
