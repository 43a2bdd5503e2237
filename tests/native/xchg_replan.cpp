// Sharded 5 Hz replanning through the adapter's MotionPlanner (include/clrrt_adapter.hpp) over the native exchange and
// its path completion (include/clrrt_xchg.h: clrrt_xchg_path_rows), no Python:
//   select       k_xchg_path_select (clrrt_xchg_selftest_path_select) against a host loop: rows bit for bit, rows moved
//   local        W host threads, one MotionPlanner each on device 0 over the in-process transport, against ONE unsharded
//                MotionPlanner running the same query sequence (commit_path, BATCH, n_iters = G x rounds): per query and
//                rank the re-init outcome, iterations, tree size, every tree header's first 148 bytes, the path ids, the
//                committed path's headers and rows bit for bit (after the completion and the CAR_TO_WORLD transform) and
//                the filtered MPC message bit for bit.  Writes the unsharded run's outputs for the Python test, which
//                compares them with the CPU oracle's.
//   mismatch     W = 2, rank 1 clears its path before the completion: both ranks get CLRRT_ESTATE at once, no rows move
//   nocompleter  W = 2, one query without a completer: every rank whose commit left rows on the other throws
//   rccl1        one rank (option shard_hook_world1) over a one-rank RCCL communicator: the completion runs its
//                collectives, moves 0 rows, and the sequence equals the unsharded one
//   span         (measurement, not a test) host time of the completion per query, from the call to the end of the work
//                it queued (the stream is idle before: clrrt_path_commit waits): span <local|rccl1> ...
// Usage: xchg_replan select
//        xchg_replan local <inputs.bin> <outputs.bin> <W> <G> <rounds> <defer_steps> <nn_lag>
//        xchg_replan mismatch|nocompleter <inputs.bin> <G> <rounds>
//        xchg_replan rccl1 <inputs.bin> <G> <rounds> <defer_steps> <nn_lag>
//        xchg_replan span <local|rccl1> <inputs.bin> <G> <rounds> <defer_steps> <nn_lag>
// inputs.bin: the per-query world state, car-frame goal and obstacles in plan_motion's CLPM format.
// Prints one line per case and "failures N" at the end; exit status 0 only with N = 0.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iterator>
#include <string>
#include <thread>
#include <vector>

#include "../../include/clrrt_adapter.hpp"
#include "../../include/clrrt_xchg.h"

namespace ad = clrrt_adapter;

static const int HDR = 148;  // clrrt_node bytes before owner / row_offset
static const uint32_t SEED = 11;

struct Query {
  std::vector<double> state;
  double goal[4];
  std::vector<clrrt_obstacle> det;
};
struct Inputs {
  int32_t coll = 0;
  std::vector<Query> q;
};

template <class T>
static T take(const char*& p) {
  T v;
  memcpy(&v, p, sizeof(T));
  p += sizeof(T);
  return v;
}
template <class T>
static void put(std::vector<char>& o, const T& v) {
  const char* b = (const char*)&v;
  o.insert(o.end(), b, b + sizeof(T));
}

static bool read_inputs(const char* path, Inputs* in) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (buf.size() < 12 || memcmp(buf.data(), "CLPM", 4) != 0) return false;
  const char* p = buf.data() + 4;
  in->coll = take<int32_t>(p);
  in->q.resize(take<int32_t>(p));
  for (auto& q : in->q) {
    q.state.resize(6);
    for (auto& v : q.state) v = take<double>(p);
    for (auto& g : q.goal) g = take<double>(p);
    q.det.resize(take<int32_t>(p));
    for (auto& o : q.det) {
      o.cx = take<double>(p); o.cy = take<double>(p); o.theta = take<double>(p);
      o.size_x = take<double>(p); o.size_y = take<double>(p); o.vx = take<double>(p); o.vy = take<double>(p);
    }
  }
  return true;
}

struct Case {
  int W, G, rounds, T, lag;
};

struct QOut {
  bool found = false;
  ad::PlanReport rep;
  ad::MPCTrajectory msg;
  std::vector<clrrt_node> tree, path;
  std::vector<double> rows;
  double span_ms = 0;  // the completion (span mode)
};
struct Run {
  int rc = CLRRT_OK;
  std::string err;
  std::vector<QOut> q;
  int64_t ps[4] = {};       // clrrt_xchg_path_stats
  int32_t completer_rc = 0;  // the last completion's status and message (mismatch)
  std::string completer_err;
  double completer_ms = 0;
};

static int slice_max(int G, int W) { return (G + W - 1) / W; }

// clrrt.dist.exchange_capacity: 2 records per sample of the slice and of its deferred samples (the ring's rounds)
static int exchange_capacity(int max_batch, int T, double sim_dt) {
  int n_steps = 0;
  while (n_steps < 20.0 / sim_dt) n_steps++;
  const int R = T > 0 ? (2 * n_steps + T - 1) / T + 2 : 1;
  return 2 * max_batch * R;
}

static ad::MotionPlanner::Config config(const Inputs& in, const Case& k, int max_batch) {
  ad::MotionPlanner::Config cfg;
  const double goal0[4] = {0, 0, 0, 0};
  clrrt_params_default(&cfg.base, 0.0, goal0, 5.0);
  cfg.base.collision_mode = in.coll;
  cfg.cap.max_nodes = 1 << 16;
  cfg.cap.max_rows = 1 << 23;  // 2 full-horizon trajectories per sample of a round, and the tree's
  cfg.cap.max_batch = max_batch;
  cfg.cap.max_obstacles = 256;
  cfg.commit_path = true;
  cfg.mode = CLRRT_MODE_BATCH;
  cfg.batch = k.G;  // the global G
  cfg.n_iters = (int64_t)k.G * k.rounds;
  return cfg;
}

static void set_options(ad::MotionPlanner& mp, const Case& k) {
  ad::check(mp.ctx(), clrrt_set_option(mp.ctx(), "defer_steps", k.T), "defer_steps");
  ad::check(mp.ctx(), clrrt_set_option(mp.ctx(), "nn_lag", k.lag), "nn_lag");
}

// the query sequence on one planner; `n_queries` of the inputs' (all when < 0)
static void run_sequence(ad::MotionPlanner& mp, const Inputs& in, int n_queries, Run* out) {
  const int nq = n_queries < 0 ? (int)in.q.size() : std::min<int>(n_queries, (int)in.q.size());
  for (int q = 0; q < nq; q++) {
    const Query& iq = in.q[q];
    ad::MotionRequest req;
    for (int i = 0; i < 4; i++) req.goal[i] = iq.goal[i];
    req.vmax = 5.0;
    mp.updateState(iq.state);
    mp.updateObstacles(iq.det);
    QOut o;
    o.found = mp.planMotion(req, &o.msg, &o.rep, nullptr);
    o.tree.resize((size_t)o.rep.tree_size);
    if (o.rep.tree_size > 0)
      ad::check(mp.ctx(), clrrt_tree_download(mp.ctx(), 0, o.rep.tree_size, o.tree.data()), "clrrt_tree_download");
    int32_t n = 0;
    int64_t nr = 0;
    ad::check(mp.ctx(), clrrt_path_size(mp.ctx(), &n, &nr), "clrrt_path_size");
    o.path.resize((size_t)n);
    o.rows.resize(10 * (size_t)nr);
    ad::check(mp.ctx(), clrrt_path_download(mp.ctx(), o.path.data(), o.rows.data()), "clrrt_path_download");
    out->q.push_back(std::move(o));
  }
}

static Run run_unsharded(const Inputs& in, const Case& k) {
  Run r;
  try {
    ad::MotionPlanner mp(config(in, k, k.G), SEED);
    set_options(mp, k);
    run_sequence(mp, in, -1, &r);
  } catch (const std::exception& e) {
    r.rc = CLRRT_EHIP;
    r.err = e.what();
  }
  return r;
}

// what a rank's completer does besides the exchange's (the tests' variations)
struct Completer {
  clrrt_xchg* x = nullptr;
  Run* run = nullptr;
  bool clear_first = false;  // mismatch: this rank's path is cleared before the completion
  bool span = false;
  std::vector<double> spans;
};
static int32_t completer_hook(void* user, clrrt_ctx* ctx, int64_t* moved) {
  Completer* c = (Completer*)user;
  if (c->clear_first) clrrt_path_commit(ctx, nullptr, 0, nullptr);
  const auto t0 = std::chrono::steady_clock::now();
  const int32_t rc = clrrt_xchg_path_rows(c->x, ctx, moved);
  if (c->span) clrrt_path_download(ctx, nullptr, nullptr);  // waits for the context's stream
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->spans.push_back(ms);
  c->run->completer_rc = rc;
  c->run->completer_ms = ms;
  c->run->completer_err = rc != 0 ? clrrt_xchg_last_error() : "";
  return rc;
}

enum Variant { PLAIN, MISMATCH, NOCOMPLETER, SPAN };

// one rank of the in-process transport (its own thread); make_x creates the rank's exchange object
static void rank_body(const Inputs& in, const Case& k, int rank, Variant var, int n_queries,
                      const std::function<int(int cap, int first_bound, clrrt_xchg**)>& make_x, bool world1, Run* out) {
  clrrt_xchg* x = nullptr;
  try {
    const int sl = slice_max(k.G, k.W);
    ad::MotionPlanner mp(config(in, k, sl), SEED);
    set_options(mp, k);
    if (world1) ad::check(mp.ctx(), clrrt_set_option(mp.ctx(), "shard_hook_world1", 1), "shard_hook_world1");
    int rc = make_x(exchange_capacity(sl, k.T, 0.04), sl, &x);
    if (rc == CLRRT_OK) rc = clrrt_xchg_attach(x, mp.ctx());
    if (rc != CLRRT_OK) throw ad::Error(std::string("exchange: ") + clrrt_xchg_last_error());
    Completer c;
    c.x = x;
    c.run = out;
    c.clear_first = var == MISMATCH && rank == 1;
    c.span = var == SPAN;
    if (var != NOCOMPLETER) mp.setPathCompleter(completer_hook, &c);
    try {
      run_sequence(mp, in, n_queries, out);
    } catch (const std::exception& e) {
      out->rc = CLRRT_ESTATE;
      out->err = e.what();
    }
    for (size_t q = 0; q < out->q.size() && q < c.spans.size(); q++) out->q[q].span_ms = c.spans[q];
    clrrt_xchg_path_stats(x, out->ps);
  } catch (const std::exception& e) {
    out->rc = CLRRT_EHIP;
    out->err = e.what();
  }
  // (the planner is gone: the exchange object outlives the context it was attached to, as in xchg_shards)
  clrrt_xchg_destroy(x);
}

static std::vector<Run> run_local(const Inputs& in, const Case& k, Variant var, int n_queries, int timeout_ms) {
  std::vector<Run> ranks(k.W);
  clrrt_xchg_group* g = nullptr;
  if (clrrt_xchg_group_create(k.W, timeout_ms, &g) != CLRRT_OK) {
    for (auto& r : ranks) { r.rc = CLRRT_EINVAL; r.err = clrrt_xchg_last_error(); }
    return ranks;
  }
  std::vector<std::thread> th;
  for (int r = 0; r < k.W; r++)
    th.emplace_back([&, r]() {
      rank_body(in, k, r, var, n_queries,
                [&, r](int cap, int fb, clrrt_xchg** x) { return clrrt_xchg_create_local(g, r, 0, cap, fb, x); }, false,
                &ranks[r]);
    });
  for (auto& t : th) t.join();
  clrrt_xchg_group_destroy(g);
  return ranks;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * 8) == 0);
}
static bool same_headers(const std::vector<clrrt_node>& a, const std::vector<clrrt_node>& b, size_t* at) {
  if (a.size() != b.size()) { *at = std::min(a.size(), b.size()); return false; }
  for (size_t i = 0; i < a.size(); i++)
    if (memcmp(&a[i], &b[i], HDR) != 0) { *at = i; return false; }
  return true;
}

// "" when rank `rank`'s sequence equals the unsharded one
static std::string compare(const Run& ref, const Run& t, int rank) {
  const std::string who = "rank " + std::to_string(rank);
  if (t.rc != CLRRT_OK) return who + " failed: " + t.err;
  if (t.q.size() != ref.q.size()) return who + ": " + std::to_string(t.q.size()) + " queries";
  for (size_t q = 0; q < ref.q.size(); q++) {
    const QOut &a = ref.q[q], &b = t.q[q];
    const std::string at = who + " query " + std::to_string(q) + ": ";
    size_t i = 0;
    if (b.rep.reinit_outcome != a.rep.reinit_outcome) return at + "re-init outcome " + std::to_string(b.rep.reinit_outcome);
    if (b.rep.iterations != a.rep.iterations) return at + "iterations differ";
    if (b.rep.tree_size != a.rep.tree_size) return at + "tree size " + std::to_string((long long)b.rep.tree_size);
    if (!same_headers(a.tree, b.tree, &i)) return at + "tree header " + std::to_string(i) + " differs";
    if (b.rep.path != a.rep.path || b.found != a.found) return at + "path ids differ";
    if (!same_headers(a.path, b.path, &i)) return at + "path header " + std::to_string(i) + " differs";
    for (size_t n = 0; n < a.path.size(); n++)
      if (a.path[n].row_offset != b.path[n].row_offset) return at + "path row layout differs";
    if (!same_bits(a.rows, b.rows)) {
      size_t r = 0;
      while (r < a.rows.size() && r < b.rows.size() && memcmp(&a.rows[r], &b.rows[r], 8) == 0) r++;
      return at + "path rows differ (row " + std::to_string(r / 10) + " of " + std::to_string(a.rows.size() / 10) + ")";
    }
    if (!same_bits(a.msg.x, b.msg.x) || !same_bits(a.msg.y, b.msg.y) || !same_bits(a.msg.theta, b.msg.theta) ||
        !same_bits(a.msg.v, b.msg.v) || !same_bits(a.msg.a, b.msg.a) || !same_bits(a.msg.a_cmd, b.msg.a_cmd) ||
        !same_bits(a.msg.d_cmd, b.msg.d_cmd) || a.msg.published != b.msg.published)
      return at + "MPC message differs";
  }
  return "";
}

// the scenario must exercise what the test is about
static std::string scenario(const Run& ref, const Case& k) {
  if (ref.rc != CLRRT_OK) return "the unsharded run failed: " + ref.err;
  int kept = 0;
  for (size_t q = 0; q < ref.q.size(); q++) {
    if (!ref.q[q].found || ref.q[q].rep.path.empty())
      return "scenario too weak: the unsharded query " + std::to_string(q) + " found no path";
    if (q >= 1 && ref.q[q].rep.reinit_outcome == CLRRT_REINIT_KEPT) kept++;
    if (k.T > 0 && ref.q[q].rep.deferred <= 0)
      return "scenario too weak: no deferred samples in query " + std::to_string(q) + " with defer_steps " + std::to_string(k.T);
  }
  if (ref.q.size() >= 4 && kept < 2) return "scenario too weak: " + std::to_string(kept) + " KEPT re-inits in queries 1-3";
  return "";
}

static void write_outputs(const char* path, const Run& ref) {
  // plan_motion's CLPO records (counters as reported, no markers)
  std::vector<char> out;
  out.insert(out.end(), {'C', 'L', 'P', 'O'});
  put(out, (int32_t)ref.q.size());
  for (const QOut& o : ref.q) {
    put(out, (int32_t)o.found);
    put(out, o.rep.reinit_outcome);
    put(out, o.rep.iterations);
    put(out, o.rep.tree_size);
    put(out, (int32_t)o.rep.path.size());
    for (int32_t id : o.rep.path) put(out, id);
    put(out, (int32_t)o.msg.published);
    put(out, (int32_t)o.msg.x.size());
    for (size_t i = 0; i < o.msg.x.size(); i++) {
      put(out, o.msg.x[i]); put(out, o.msg.y[i]); put(out, o.msg.theta[i]); put(out, o.msg.v[i]);
      put(out, o.msg.a[i]); put(out, o.msg.a_cmd[i]); put(out, o.msg.d_cmd[i]);
    }
    for (int c = 0; c < 4; c++) put(out, o.rep.counters[c]);
    put(out, (int32_t)0);
    put(out, o.rep.deferred);
    put(out, (int64_t)(o.rows.size() / 10));
  }
  std::ofstream f(path, std::ios::binary);
  f.write(out.data(), (std::streamsize)out.size());
}

static std::string describe(const Run& ref) {
  std::string s;
  for (const QOut& o : ref.q)
    s += (s.empty() ? "" : " | ") + std::string("oc ") + std::to_string(o.rep.reinit_outcome) + " tree " +
         std::to_string((long long)o.rep.tree_size) + " path " + std::to_string(o.rep.path.size()) + "/" +
         std::to_string(o.rows.size() / 10) + " rows, deferred " + std::to_string((long long)o.rep.deferred);
  return s;
}

static int check_ranks(const char* name, const Case& k, const Run& ref, const std::vector<Run>& ranks, bool want_fetch) {
  std::string why = scenario(ref, k);
  for (int r = 0; r < (int)ranks.size() && why.empty(); r++) why = compare(ref, ranks[r], r);
  std::string fetched;
  for (size_t q = 0; q < ref.q.size() && why.empty(); q++) {
    int64_t sum = 0;
    for (const Run& t : ranks) sum += t.q[q].rep.rows_fetched;
    fetched += (fetched.empty() ? "" : ",") + std::to_string((long long)sum);
    if (want_fetch && sum <= 0) why = "no rows fetched in query " + std::to_string(q);
    if (!want_fetch && sum != 0) why = "rows fetched in query " + std::to_string(q);
  }
  for (int r = 0; r < (int)ranks.size() && why.empty(); r++) {
    const Run& t = ranks[r];
    if (t.ps[0] != (int64_t)ref.q.size()) why = "rank " + std::to_string(r) + ": " + std::to_string((long long)t.ps[0]) + " completions";
    else if (t.ps[1] <= 0) why = "rank " + std::to_string(r) + ": no collective";
  }
  printf("%s W=%d G=%d rounds=%d T=%d lag=%d: %s; rows fetched per query (all ranks) %s; rank 0 completions %lld "
         "collectives %lld rows gathered %lld taken %lld: %s\n",
         name, k.W, k.G, k.rounds, k.T, k.lag, describe(ref).c_str(), fetched.c_str(), (long long)ranks[0].ps[0],
         (long long)ranks[0].ps[1], (long long)ranks[0].ps[2], (long long)ranks[0].ps[3],
         why.empty() ? "ok" : ("FAILED: " + why).c_str());
  return why.empty() ? 0 : 1;
}

static int mode_local(const Inputs& in, const char* out_path, const Case& k) {
  const Run ref = run_unsharded(in, k);
  if (ref.rc == CLRRT_OK) write_outputs(out_path, ref);
  return check_ranks("local", k, ref, run_local(in, k, PLAIN, -1, 60000), true);
}

static int mode_mismatch(const Inputs& in, int G, int rounds) {
  const Case k{2, G, rounds, 0, 1};
  const std::vector<Run> r = run_local(in, k, MISMATCH, 1, 60000);
  bool ok = true;
  for (const Run& t : r)
    ok = ok && t.rc == CLRRT_ESTATE && t.completer_rc == CLRRT_ESTATE && t.completer_ms < 10000 && t.ps[2] == 0 &&
         t.ps[3] == 0 && t.completer_err.find("rank 1") != std::string::npos;
  printf("mismatch rank 1 cleared its path: rank 0 (%d, %.1f ms) '%s', rank 1 (%d, %.1f ms) '%s'; rows gathered %lld/%lld: %s\n",
         r[0].completer_rc, r[0].completer_ms, r[0].completer_err.c_str(), r[1].completer_rc, r[1].completer_ms,
         r[1].completer_err.c_str(), (long long)r[0].ps[2], (long long)r[1].ps[2], ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

static int mode_nocompleter(const Inputs& in, int G, int rounds) {
  const Case k{2, G, rounds, 0, 1};
  const std::vector<Run> r = run_local(in, k, NOCOMPLETER, 1, 60000);
  int threw = 0;
  bool ok = true;
  for (const Run& t : r) {
    if (t.rc == CLRRT_OK) {
      // no rows on the other rank: every node of its path must be its own
      ok = ok && t.q.size() == 1;
    } else {
      ok = ok && t.rc == CLRRT_ESTATE && t.err.find("no path completer") != std::string::npos;
      threw++;
    }
  }
  ok = ok && threw >= 1;
  printf("nocompleter: rank 0 (%d) '%s', rank 1 (%d) '%s': %s\n", r[0].rc, r[0].err.c_str(), r[1].rc, r[1].err.c_str(),
         ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

// 0 ran, 1 failed, 2 skipped (the machine could not make a communicator)
static int rccl_run(const Inputs& in, const Case& k, Variant var, Run* out) {
  unsigned char uid[CLRRT_XCHG_UID_BYTES];
  if (clrrt_xchg_unique_id(uid) != CLRRT_OK) {
    const std::string e = clrrt_xchg_last_error();
    printf("rccl1: %s: %s\n", e.find("ncclSystemError") != std::string::npos ? "SKIPPED, no communicator on this machine" : "FAILED", e.c_str());
    return e.find("ncclSystemError") != std::string::npos ? 2 : 1;
  }
  bool skipped = false;
  rank_body(in, k, 0, var, -1,
            [&](int cap, int fb, clrrt_xchg** x) {
              const int rc = clrrt_xchg_create_rccl(uid, 0, 1, 0, cap, fb, x);
              if (rc != CLRRT_OK && std::string(clrrt_xchg_last_error()).find("ncclSystemError") != std::string::npos)
                skipped = true;
              return rc;
            },
            true, out);
  if (skipped) {
    printf("rccl1: SKIPPED, no communicator on this machine: %s\n", out->err.c_str());
    return 2;
  }
  return 0;
}

static int mode_rccl1(const Inputs& in, const Case& k) {
  std::vector<Run> ranks(1);
  const int s = rccl_run(in, k, PLAIN, &ranks[0]);
  if (s == 2) { printf("skipped rccl1\n"); return 0; }
  if (s == 1) return 1;
  return check_ranks("rccl1", k, run_unsharded(in, k), ranks, false);
}

static int mode_span(const char* transport, const Inputs& in, const Case& k) {
  const bool local = strcmp(transport, "local") == 0;
  std::vector<Run> ranks;
  for (int rep = 0; rep < 2; rep++) {  // the first run loads the code objects
    if (local) ranks = run_local(in, k, SPAN, -1, 60000);
    else {
      ranks.assign(1, Run());
      if (rccl_run(in, k, SPAN, &ranks[0]) != 0) return 1;
    }
  }
  for (size_t r = 0; r < ranks.size(); r++) {
    const Run& t = ranks[r];
    if (t.rc != CLRRT_OK) { printf("span: rank %zu failed: %s\n", r, t.err.c_str()); return 1; }
    for (size_t q = 0; q < t.q.size(); q++)
      printf("span %s W=%d G=%d rounds=%d T=%d lag=%d rank %zu query %zu: completion %.1f us (path %zu nodes, %zu rows, "
             "%lld rows taken)\n", transport, k.W, k.G, k.rounds, k.T, k.lag, r, q, 1e3 * t.q[q].span_ms, t.q[q].path.size(),
             t.q[q].rows.size() / 10, (long long)t.q[q].rep.rows_fetched);
  }
  return 0;
}

// ---- select: the kernel against a host loop
static uint64_t pattern(int r, int64_t j, int c) {
  const uint64_t b = ((uint64_t)(r + 1) << 44) | ((uint64_t)j << 8) | (uint64_t)c;
  switch ((j + c) % 5) {
    case 1: return 0x7FF8000000000000ull | b;
    case 2: return 0xFFF0000000000000ull | b;
    case 3: return 0x8000000000000000ull;
    case 4: return 0x4000000000000000ull | b;
    default: return b;
  }
}

static int select_case(int W, int self, const std::vector<int32_t>& owners, const std::vector<int32_t>& nrows) {
  const int n = (int)owners.size();
  int64_t R = 0;
  for (int v : nrows) R += v;
  std::vector<uint64_t> got((size_t)std::max<int64_t>(R, 1) * 10, 0xEEEEEEEEEEEEEEEEull), want((size_t)R * 10);
  int64_t moved = -1, wmoved = 0, j = 0;
  for (int i = 0; i < n; i++) {
    for (int q = 0; q < nrows[i]; q++, j++)
      for (int c = 0; c < 10; c++) want[(size_t)j * 10 + c] = pattern(owners[i], j, c);  // own nodes: its own pattern
    if (owners[i] != self) wmoved += nrows[i];
  }
  const int rc = clrrt_xchg_selftest_path_select(0, W, self, n, owners.data(), nrows.data(), got.data(), &moved);
  std::string why;
  if (rc != CLRRT_OK) why = std::string("selftest -> ") + std::to_string(rc) + " " + clrrt_xchg_last_error();
  else if (R > 0 && memcmp(got.data(), want.data(), want.size() * 8) != 0) why = "rows differ";
  else if (moved != wmoved) why = "moved " + std::to_string((long long)moved) + ", expected " + std::to_string((long long)wmoved);
  printf("select W=%d self=%d n=%d rows=%lld moved=%lld: %s\n", W, self, n, (long long)R, (long long)wmoved,
         why.empty() ? "ok" : ("FAILED: " + why).c_str());
  return why.empty() ? 0 : 1;
}

static int mode_select() {
  int bad = 0;
  bad += select_case(1, 0, {0}, {1});
  bad += select_case(1, 0, {}, {});
  bad += select_case(2, 0, {0, 1}, {1, 1});
  bad += select_case(2, 1, {1, 1, 1}, {3, 1, 2});  // nothing moves: the rank's own rows are untouched
  for (int self = 0; self < 3; self++) bad += select_case(3, self, {2, 0, 1, 2, 0}, {501, 1, 64, 2, 163});
  {
    std::vector<int32_t> ow(300), nr(300, 1);  // more nodes than a block has threads
    for (int i = 0; i < 300; i++) ow[i] = i % 8;
    bad += select_case(8, 3, ow, nr);
  }
  {
    std::vector<int32_t> ow(64), nr(64, 3);
    for (int i = 0; i < 64; i++) ow[i] = i;
    bad += select_case(64, 17, ow, nr);
  }
  return bad;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  int bad = 0;
  Inputs in;
  auto need = [&](int n, const char* file) {
    if (argc < n) { fprintf(stderr, "xchg_replan %s: too few arguments (see the head of xchg_replan.cpp)\n", mode.c_str()); exit(2); }
    if (!read_inputs(file, &in) || in.q.empty()) { fprintf(stderr, "bad inputs %s\n", file); exit(2); }
  };
  if (mode == "select") bad = mode_select();
  else if (mode == "local") {
    need(9, argc > 2 ? argv[2] : "");
    bad = mode_local(in, argv[3], Case{atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8])});
  } else if (mode == "mismatch" || mode == "nocompleter") {
    need(5, argc > 2 ? argv[2] : "");
    bad = mode == "mismatch" ? mode_mismatch(in, atoi(argv[3]), atoi(argv[4])) : mode_nocompleter(in, atoi(argv[3]), atoi(argv[4]));
  } else if (mode == "rccl1") {
    need(7, argc > 2 ? argv[2] : "");
    bad = mode_rccl1(in, Case{1, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])});
  } else if (mode == "span") {
    need(8, argc > 3 ? argv[3] : "");
    const bool local = strcmp(argv[2], "local") == 0;
    return mode_span(argv[2], in, Case{local ? 2 : 1, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7])});
  } else {
    fprintf(stderr, "usage: %s <select|local|mismatch|nocompleter|rccl1|span> ... (see the head of xchg_replan.cpp)\n", argv[0]);
    return 2;
  }
  printf("failures %d\n", bad);
  return bad ? 1 : 0;
}
