// Sharded clrrt_expand through the native exchange (include/clrrt_xchg.h, libclrrt_xchg.so), no Python:
//   local    W host threads, each with its own context on device 0 and the in-process transport, against one
//            unsharded context: every rank's tree must equal it (the first 148 bytes of every header, each node's rows
//            on its owner, iterations, goal nodes, the sum of the ranks' deferred samples), one closing exchange per
//            rank, collectives == exchanges with the bound at the slice size, second gathers > 0 with a bound of 8
//   rccl1    one rank, option shard_hook_world1, a one-rank RCCL communicator (G = 1024, defer_steps 48, 8 rounds): the
//            same comparison
//   failure  local W = 2 with fail_at_round 2 on rank 1 (both ranks must fail, each with its own message), and a
//            world-2 group whose second rank never runs (CLRRT_EHIP within the group's deadline)
//   concat   k_xchg_concat (clrrt_xchg_selftest_concat) against a host loop, rows and summary bit for bit
//   span     (measurement, not a test) the exchange's stream span per round: span <local|rccl1> <G> <rounds>
// Usage: xchg_shards <mode> <obstacles.bin> [case index | span arguments]
// Prints one line per case and "failures N" at the end; exit status 0 only with N = 0.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <thread>
#include <vector>

#include "../../include/clrrt_xchg.h"

static std::vector<clrrt_obstacle> g_obs;
static const int HDR = 148;  // clrrt_node bytes before owner / row_offset
static const uint32_t SEED = 17;

struct Tree {
  int rc = CLRRT_OK;
  std::string err;
  clrrt_stats st{};
  std::vector<clrrt_node> nodes;
  std::vector<std::vector<double>> rows;  // of the nodes this rank owns (empty otherwise)
  int64_t xs[8] = {};
  double span_ms = 0;
  int64_t span_n = 0;
  double wall_ms = 0;
};

struct Case {
  int W, G, T, lag, rounds, first_bound;  // first_bound 0: the slice size
};

static int slice_max(int G, int W) { return (G + W - 1) / W; }

// clrrt.dist.exchange_capacity: 2 records per sample of the slice and of its deferred samples (the ring's rounds)
static int exchange_capacity(int max_batch, int T, double sim_dt) {
  int n_steps = 0;
  while (n_steps < 20.0 / sim_dt) n_steps++;
  const int R = T > 0 ? (2 * n_steps + T - 1) / T + 2 : 1;
  return 2 * max_batch * R;
}

static clrrt_params params() {
  clrrt_params p;
  const double goal[4] = {40, 0, 0, 0};
  clrrt_params_default(&p, 0.0, goal, 5.0);
  p.collision_mode = CLRRT_COLLISION_OBB;
  return p;
}

static clrrt_ctx* make_ctx(int max_batch, int T, int lag, std::string* err) {
  const clrrt_params p = params();
  // (the arena check wants room for 2 full-horizon trajectories per sample of a round: the span mode's large rounds)
  clrrt_capacity cap{1 << 18, max_batch > 8192 ? 1 << 26 : 1 << 24, max_batch, 256};
  clrrt_ctx* c = nullptr;
  if (clrrt_create(&p, &cap, 0, &c) != CLRRT_OK) { *err = "clrrt_create failed"; return nullptr; }
  const double root[10] = {0};
  if (clrrt_set_obstacles(c, g_obs.data(), (int32_t)g_obs.size()) != CLRRT_OK || clrrt_tree_init(c, root) != CLRRT_OK ||
      clrrt_set_option(c, "defer_steps", T) != CLRRT_OK || clrrt_set_option(c, "nn_lag", lag) != CLRRT_OK ||
      clrrt_set_option(c, "nn_walk_min", 64) != CLRRT_OK) {
    *err = std::string("context setup: ") + clrrt_last_error(c);
    clrrt_destroy(c);
    return nullptr;
  }
  return c;
}

// expands and snapshots the tree (the rows of the nodes `rank` owns; rank < 0: of every node)
static void expand_and_snapshot(clrrt_ctx* c, const Case& k, int rank, Tree* t, bool timing = false) {
  clrrt_rng rng;
  clrrt_rng_seed(&rng, SEED);
  if (timing) clrrt_enable_timing(c, 1);
  const auto t0 = std::chrono::steady_clock::now();
  t->rc = clrrt_expand(c, &rng, (int64_t)k.rounds * k.G, 0.0, CLRRT_MODE_BATCH, k.G, &t->st);
  t->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (t->rc != CLRRT_OK) { t->err = clrrt_last_error(c); return; }
  if (timing) clrrt_kernel_time(c, 5, &t->span_ms, &t->span_n);
  int64_t n = 0, nr = 0;
  clrrt_tree_size(c, &n, &nr);
  t->nodes.resize(n);
  t->rows.resize(n);
  if (clrrt_tree_download(c, 0, n, t->nodes.data()) != CLRRT_OK) { t->rc = CLRRT_EHIP; t->err = "download"; return; }
  for (int64_t i = 0; i < n; i++) {
    const clrrt_node& nd = t->nodes[i];
    if (rank >= 0 && nd.owner != rank) continue;
    t->rows[i].resize((size_t)nd.nrows * 10);
    if (nd.nrows > 0 && clrrt_tree_rows(c, nd.row_offset, nd.nrows, t->rows[i].data()) != CLRRT_OK) {
      t->rc = CLRRT_EHIP;
      t->err = std::string("rows: ") + clrrt_last_error(c);
      return;
    }
  }
}

static Tree run_reference(const Case& k) {
  Tree t;
  clrrt_ctx* c = make_ctx(k.G, k.T, k.lag, &t.err);
  if (!c) { t.rc = CLRRT_EHIP; return t; }
  expand_and_snapshot(c, k, -1, &t);
  clrrt_destroy(c);
  return t;
}

// one rank of the in-process transport (its own thread)
static void local_rank(clrrt_xchg_group* g, const Case& k, int rank, int fail_round, Tree* t, bool timing) {
  clrrt_ctx* c = make_ctx(slice_max(k.G, k.W), k.T, k.lag, &t->err);
  if (!c) { t->rc = CLRRT_EHIP; return; }
  const int sl = slice_max(k.G, k.W);
  clrrt_xchg* x = nullptr;
  t->rc = clrrt_xchg_create_local(g, rank, 0, exchange_capacity(sl, k.T, params().sim_dt),
                                  k.first_bound ? k.first_bound : sl, &x);
  if (t->rc == CLRRT_OK) t->rc = clrrt_xchg_attach(x, c);
  if (t->rc != CLRRT_OK) {
    t->err = clrrt_xchg_last_error();
  } else {
    if (fail_round > 0) clrrt_set_option(c, "fail_at_round", fail_round);
    expand_and_snapshot(c, k, rank, t, timing);
    clrrt_xchg_stats(x, t->xs);
  }
  clrrt_destroy(c);
  clrrt_xchg_destroy(x);
}

// "" when rank `rank`'s tree equals the reference's
static std::string compare(const Tree& ref, const Tree& t, int rank, int64_t* owned) {
  if (t.rc != CLRRT_OK) return "rank " + std::to_string(rank) + " failed: " + t.err;
  if (t.nodes.size() != ref.nodes.size())
    return "rank " + std::to_string(rank) + ": " + std::to_string(t.nodes.size()) + " nodes, reference " +
           std::to_string(ref.nodes.size());
  for (size_t i = 0; i < ref.nodes.size(); i++) {
    if (memcmp(&t.nodes[i], &ref.nodes[i], HDR) != 0)
      return "rank " + std::to_string(rank) + ": header of node " + std::to_string(i) + " differs";
    if (t.nodes[i].owner != rank) continue;
    (*owned)++;
    if (t.nodes[i].nrows != ref.nodes[i].nrows || t.rows[i].size() != ref.rows[i].size() ||
        memcmp(t.rows[i].data(), ref.rows[i].data(), t.rows[i].size() * 8) != 0)
      return "rank " + std::to_string(rank) + ": rows of node " + std::to_string(i) + " differ";
  }
  if (t.st.iterations != ref.st.iterations) return "rank " + std::to_string(rank) + ": iterations differ";
  if (t.st.goal_nodes_added != ref.st.goal_nodes_added) return "rank " + std::to_string(rank) + ": goal nodes differ";
  return "";
}

static int check_against_reference(const char* name, const Case& k, const Tree& ref, const std::vector<Tree>& ranks) {
  std::string why;
  if (ref.rc != CLRRT_OK) why = "reference failed: " + ref.err;
  else if (ref.nodes.size() <= 2000) why = "the reference tree has only " + std::to_string(ref.nodes.size()) + " nodes";
  else if (k.T > 0 && ref.st.deferred <= 0) why = "no deferred samples with defer_steps " + std::to_string(k.T);
  int64_t owned = 0, deferred = 0;
  for (int r = 0; r < (int)ranks.size() && why.empty(); r++) {
    const Tree& t = ranks[r];
    why = compare(ref, t, r, &owned);
    if (!why.empty()) break;
    deferred += t.st.deferred;
    if (t.xs[3] != 1) why = "rank " + std::to_string(r) + ": " + std::to_string(t.xs[3]) + " closing exchanges";
    else if (t.xs[0] < k.rounds + 1) why = "rank " + std::to_string(r) + ": fewer exchanges than rounds + 1";
    else if (k.first_bound == 0 && t.xs[1] != t.xs[0]) why = "rank " + std::to_string(r) + ": collectives != exchanges";
    else if (k.first_bound != 0 && t.xs[2] <= 0) why = "rank " + std::to_string(r) + ": no second gather";
  }
  if (why.empty() && owned != (int64_t)ref.nodes.size()) why = "the ranks own " + std::to_string(owned) + " nodes";
  if (why.empty() && deferred != ref.st.deferred) why = "deferred samples differ from the reference's";
  printf("%s W=%d G=%d T=%d lag=%d rounds=%d first_bound=%d: %zu nodes, deferred %lld, goals %lld; exchanges %lld "
         "collectives %lld second gathers %lld rows sent (rank 0) %lld received %lld: %s\n",
         name, k.W, k.G, k.T, k.lag, k.rounds, k.first_bound, ref.nodes.size(), (long long)ref.st.deferred,
         (long long)ref.st.goal_nodes_added, (long long)ranks[0].xs[0], (long long)ranks[0].xs[1],
         (long long)ranks[0].xs[2], (long long)ranks[0].xs[4], (long long)ranks[0].xs[5],
         why.empty() ? "ok" : ("FAILED: " + why).c_str());
  return why.empty() ? 0 : 1;
}

static std::vector<Tree> run_local(const Case& k, int timeout_ms, int fail_rank, int fail_round, bool timing = false) {
  std::vector<Tree> ranks(k.W);
  clrrt_xchg_group* g = nullptr;
  if (clrrt_xchg_group_create(k.W, timeout_ms, &g) != CLRRT_OK) {
    for (auto& t : ranks) { t.rc = CLRRT_EINVAL; t.err = clrrt_xchg_last_error(); }
    return ranks;
  }
  std::vector<std::thread> th;
  for (int r = 0; r < k.W; r++)
    th.emplace_back(local_rank, g, std::cref(k), r, r == fail_rank ? fail_round : 0, &ranks[r], timing);
  for (auto& t : th) t.join();
  clrrt_xchg_group_destroy(g);
  return ranks;
}

static const Case LOCAL_CASES[] = {
    {2, 2048, 0, 1, 4, 0},
    {3, 3065, 48, 1, 4, 0},  // uneven slices
    {2, 2048, 64, 2, 6, 0},
    {2, 2048, 0, 1, 4, 8},   // the first rounds need the second gather (then the bound has adapted)
};

static int mode_local(int only) {
  int bad = 0;
  for (int i = 0; i < 4; i++) {
    if (only >= 0 && only != i) continue;
    const Case& k = LOCAL_CASES[i];
    const Tree ref = run_reference(k);
    bad += check_against_reference("local", k, ref, run_local(k, 60000, -1, 0));
  }
  return bad;
}

// 0 ok, 1 failed, 2 skipped (the machine could not make a communicator)
static int rccl_rank(const Case& k, Tree* t, bool timing) {
  unsigned char uid[CLRRT_XCHG_UID_BYTES];
  clrrt_xchg* x = nullptr;
  int rc = clrrt_xchg_unique_id(uid);
  const int sl = k.G;
  if (rc == CLRRT_OK)
    rc = clrrt_xchg_create_rccl(uid, 0, 1, 0, exchange_capacity(sl, k.T, params().sim_dt), sl, &x);
  if (rc != CLRRT_OK) {
    const std::string e = clrrt_xchg_last_error();
    if (e.find("ncclSystemError") != std::string::npos) {
      printf("rccl1: SKIPPED, no communicator on this machine: %s\n", e.c_str());
      return 2;
    }
    printf("rccl1: FAILED: %s\n", e.c_str());
    return 1;
  }
  clrrt_ctx* c = make_ctx(k.G, k.T, k.lag, &t->err);
  if (!c) { printf("rccl1: FAILED: %s\n", t->err.c_str()); clrrt_xchg_destroy(x); return 1; }
  clrrt_set_option(c, "shard_hook_world1", 1);
  t->rc = clrrt_xchg_attach(x, c);
  if (t->rc != CLRRT_OK) t->err = clrrt_xchg_last_error();
  else {
    expand_and_snapshot(c, k, 0, t, timing);
    clrrt_xchg_stats(x, t->xs);
  }
  clrrt_destroy(c);
  clrrt_xchg_destroy(x);
  return 0;
}

static int mode_rccl1() {
  // (8 rounds, not 4: at G = 1024 with defer_steps 48 four rounds grow ~1200 nodes, fewer than the 2000 asked for)
  const Case k{1, 1024, 48, 1, 8, 0};
  std::vector<Tree> ranks(1);
  const int s = rccl_rank(k, &ranks[0], false);
  if (s == 2) { printf("skipped rccl1\n"); return 0; }
  if (s == 1) return 1;
  return check_against_reference("rccl1", k, run_reference(k), ranks);
}

static int mode_failure() {
  int bad = 0;
  {
    const Case k{2, 2048, 48, 1, 4, 0};
    const std::vector<Tree> r = run_local(k, 60000, 1, 2);
    const bool ok = r[0].rc != CLRRT_OK && r[1].rc != CLRRT_OK && r[1].err.find("injected failure") != std::string::npos &&
                    r[0].err.find("rank(s) failed") != std::string::npos;
    printf("failure fail_at_round 2 on rank 1: rank 0 (%d) '%s', rank 1 (%d) '%s': %s\n", r[0].rc, r[0].err.c_str(),
           r[1].rc, r[1].err.c_str(), ok ? "ok" : "FAILED");
    bad += !ok;
  }
  {
    // a world of 2 whose rank 1 never runs: rank 0's first exchange gives up at the deadline
    const Case k{2, 2048, 0, 1, 4, 0};
    clrrt_xchg_group* g = nullptr;
    Tree t;
    double ms = 0;
    if (clrrt_xchg_group_create(2, 500, &g) == CLRRT_OK) {
      const auto t0 = std::chrono::steady_clock::now();
      std::thread th(local_rank, g, std::cref(k), 0, 0, &t, false);
      th.join();
      ms = t.wall_ms;
      (void)t0;
      clrrt_xchg_group_destroy(g);
    }
    const bool ok = t.rc == CLRRT_EHIP && ms >= 400 && ms < 5000;
    printf("failure missing peer: clrrt_expand -> %d '%s' after %.0f ms: %s\n", t.rc, t.err.c_str(), ms,
           ok ? "ok" : "FAILED");
    bad += !ok;
  }
  return bad;
}

static int concat_case(int W, int bound, std::vector<int32_t> counts) {
  int maxc = 0;
  int64_t total = 0;
  for (int c : counts) { maxc = std::max(maxc, c); total += c; }
  const int ex = std::max(0, maxc - bound);
  std::vector<double> elapsed(W), bbox(4 * W);
  std::vector<int64_t> aux(W);
  for (int r = 0; r < W; r++) {
    elapsed[r] = 3.25 + ((r * 5) % 7) * 0.125;
    aux[r] = (int64_t)r * 3 + ((r == 1) ? (1ll << 32) : 0) + ((r == W - 1) ? (1ll << 48) : 0);
    if (counts[r] == 0) {
      bbox[4 * r] = bbox[4 * r + 1] = HUGE_VAL;
      bbox[4 * r + 2] = bbox[4 * r + 3] = -HUGE_VAL;
    } else {
      bbox[4 * r] = -1.5 - r; bbox[4 * r + 1] = 0.25 * ((r * 3) % 5) - 2;
      bbox[4 * r + 2] = 10.0 + ((r * 7) % 4); bbox[4 * r + 3] = 3.0 + r * 0.5;
    }
  }
  std::vector<unsigned char> got((size_t)std::max<int64_t>(total, 1) * 160, 0xEE), want((size_t)total * 160);
  std::vector<int64_t> sum(8 + W, -1), wsum(8 + W, 0);
  const int rc = clrrt_xchg_selftest_concat(0, W, bound, counts.data(), elapsed.data(), aux.data(), bbox.data(), ex,
                                            got.data(), total, sum.data());
  // the host loop
  double me = -HUGE_VAL, bb[4] = {HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  size_t o = 0;
  for (int r = 0; r < W; r++) {
    for (int j = 0; j < counts[r]; j++)
      for (int b = 0; b < 160; b++) want[o++] = (unsigned char)(r * 131 + j * 7 + b * 3 + 1);
    wsum[0] += counts[r];
    wsum[1] = std::max<int64_t>(wsum[1], counts[r]);
    me = std::max(me, elapsed[r]);
    wsum[3] += aux[r];
    bb[0] = std::min(bb[0], bbox[4 * r]); bb[1] = std::min(bb[1], bbox[4 * r + 1]);
    bb[2] = std::max(bb[2], bbox[4 * r + 2]); bb[3] = std::max(bb[3], bbox[4 * r + 3]);
    wsum[8 + r] = counts[r];
  }
  memcpy(&wsum[2], &me, 8);
  memcpy(&wsum[4], bb, 32);
  std::string why;
  if (rc != CLRRT_OK) why = std::string("selftest -> ") + std::to_string(rc) + " " + clrrt_xchg_last_error();
  else if (total > 0 && memcmp(got.data(), want.data(), want.size()) != 0) why = "rows differ";
  else if (memcmp(sum.data(), wsum.data(), 8 * (8 + W)) != 0) why = "summary differs";
  std::string cs;
  for (int c : counts) cs += (cs.empty() ? "" : ",") + std::to_string(c);
  printf("concat W=%d bound=%d counts (%s) excess rows %d: %s\n", W, bound, cs.c_str(), ex,
         why.empty() ? "ok" : ("FAILED: " + why).c_str());
  return why.empty() ? 0 : 1;
}

static int mode_concat() {
  int bad = 0;
  bad += concat_case(1, 4, {0});
  bad += concat_case(1, 4, {1});
  bad += concat_case(2, 4, {0, 0});
  bad += concat_case(2, 4, {4, 7});
  bad += concat_case(2, 4, {1, 0});
  bad += concat_case(8, 16, {0, 16, 3, 17, 1, 0, 40, 16});
  return bad;
}

static int mode_span(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "span <local|rccl1> <G> <rounds>\n"); return 1; }
  const bool local = strcmp(argv[3], "local") == 0;
  const Case k{local ? 2 : 1, atoi(argv[4]), 0, 1, atoi(argv[5]), 0};
  std::vector<Tree> ranks;
  for (int rep = 0; rep < 2; rep++) {  // the first run loads the code objects
    if (local) ranks = run_local(k, 60000, -1, 0, true);
    else {
      ranks.assign(1, Tree());
      if (rccl_rank(k, &ranks[0], true) != 0) return 1;
    }
  }
  for (size_t r = 0; r < ranks.size(); r++) {
    const Tree& t = ranks[r];
    if (t.rc != CLRRT_OK) { printf("span: rank %zu failed: %s\n", r, t.err.c_str()); return 1; }
    printf("span %s G=%d rounds=%d rank %zu: %lld exchanges timed, %.3f ms in all, %.1f us per exchange; %zu nodes, "
           "rows received %lld, expand %.1f ms\n", argv[3], k.G, k.rounds, r, (long long)t.span_n, t.span_ms,
           t.span_n ? 1e3 * t.span_ms / t.span_n : 0.0, t.nodes.size(), (long long)t.xs[5], t.wall_ms);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <local|rccl1|failure|concat|span> obstacles.bin [case]\n", argv[0]); return 2; }
  std::ifstream f(argv[2], std::ios::binary);
  std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  g_obs.resize(buf.size() / sizeof(clrrt_obstacle));
  memcpy(g_obs.data(), buf.data(), g_obs.size() * sizeof(clrrt_obstacle));
  const std::string mode = argv[1];
  int bad = 0;
  if (mode == "local") bad = mode_local(argc > 3 ? atoi(argv[3]) : -1);
  else if (mode == "rccl1") bad = mode_rccl1();
  else if (mode == "failure") bad = mode_failure();
  else if (mode == "concat") bad = mode_concat();
  else if (mode == "span") return mode_span(argc, argv);
  else { fprintf(stderr, "unknown mode %s\n", argv[1]); return 2; }
  printf("failures %d\n", bad);
  return bad ? 1 : 0;
}
