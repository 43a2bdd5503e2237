// The in-process exchange's host rendezvous (cl-rrt_amd/csrc/clrrt_rendezvous.hpp) on its own: no HIP, no library.
// Threads use it the way the exchange hook does -- publish a slot, meet, read every peer's slot, meet again, go on --
// for W = 2, 3 and 8 threads over 1000 rounds, then one group whose peer never arrives (the waiter must come back
// with false near the deadline, and a late caller at once).  tests/test_xchg_host.py builds it with
// -fsanitize=thread and expects a clean exit.
// Usage: rendezvous_check [rounds]
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../cl-rrt_amd/csrc/clrrt_rendezvous.hpp"

using clrrt_xchg_detail::Rendezvous;

static int run_group(int W, int rounds) {
  Rendezvous rv(W, 20000);
  std::vector<long long> slot(W, -1);  // plain memory: the meetings are what orders the accesses
  std::atomic<int> bad{0};
  std::vector<std::thread> th;
  for (int r = 0; r < W; r++)
    th.emplace_back([&, r] {
      for (int k = 0; k < rounds; k++) {
        slot[r] = (long long)k * 64 + r;  // "my rows are written"
        if (!rv.meet()) { bad++; return; }
        for (int p = 0; p < W; p++)  // "pull every peer's rows"
          if (slot[p] != (long long)k * 64 + p) bad++;
        if (!rv.meet()) { bad++; return; }  // the owners go on only after every puller has read
      }
    });
  for (auto& t : th) t.join();
  if (rv.generation() != 2ull * rounds) bad++;
  printf("rendezvous W=%d rounds=%d: %s\n", W, rounds, bad.load() ? "FAILED" : "ok");
  return bad.load();
}

static int run_timeout() {
  Rendezvous rv(2, 300);
  const auto t0 = std::chrono::steady_clock::now();
  bool got = true;
  std::thread t([&] { got = rv.meet(); });
  t.join();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const auto t1 = std::chrono::steady_clock::now();
  const bool late = rv.meet();  // the peer arrives after the waiter gave up: no wait, no success
  const double ms_late = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  const bool ok = !got && !late && rv.broken() && ms >= 290 && ms < 5000 && ms_late < 200;
  printf("rendezvous missing peer: waiter %s after %.0f ms, late caller %s after %.1f ms: %s\n", got ? "true" : "false",
         ms, late ? "true" : "false", ms_late, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 1000;
  int bad = 0;
  for (int W : {2, 3, 8}) bad += run_group(W, rounds);
  bad += run_timeout();
  printf("failures %d\n", bad);
  return bad ? 1 : 0;
}
