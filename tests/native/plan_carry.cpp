// Three 5 Hz planMotion queries that keep their tree (MotionPlanner::Config::carry_tree, clrrt_tree_rebase) through
// include/clrrt_adapter.hpp, linked against libclrrt (no Python): six static boxes in the world frame, handed to each
// query in the car frame.  Prints, per query, the re-init outcome, whether the tree was carried, the rebase counts, the
// tree size before and after the expansion, the committed path's ids and an FNV-1a of its rows (world frame);
// tests/test_native_plan_carry.py runs the same queries through the Python binding's replanning backend and compares.
// Usage: plan_carry <seed> <batch> <rounds> <carry 0|1>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/clrrt_adapter.hpp"

static uint64_t fnv1a(const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

// The world (the test holds the same table): cx, cy, theta, size_x, size_y, vx, vy.
static const double kBoxes[6][7] = {{12.0, 4.5, 0.3, 3.0, 1.5, 0, 0},  {18.0, -4.0, -0.2, 2.5, 1.5, 0, 0},
                                    {25.0, 3.0, 0.0, 2.0, 2.0, 0, 0},  {30.0, -3.5, 0.5, 3.0, 1.0, 0, 0},
                                    {8.0, -6.0, 0.0, 4.0, 1.0, 0, 0},  {35.0, 6.0, 0.1, 2.0, 2.0, 0, 0}};

// replan.obstacles_in_car_frame for static boxes: centre through transformPointWorldToCar, heading - pose heading.
static std::vector<clrrt_obstacle> boxes_in_car_frame(const double pose[3]) {
  const double c = std::cos(pose[2]), s = std::sin(pose[2]);
  std::vector<clrrt_obstacle> out;
  for (const auto& b : kBoxes) {
    clrrt_obstacle o;
    o.cx = b[0] * c - pose[0] * c - pose[1] * s + b[1] * s;
    o.cy = b[1] * c - pose[1] * c + pose[0] * s - b[0] * s;
    o.theta = b[2] - pose[2];
    o.size_x = b[3]; o.size_y = b[4];
    o.vx = c * b[5] + s * b[6];
    o.vy = -s * b[5] + c * b[6];
    out.push_back(o);
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s seed batch rounds carry\n", argv[0]);
    return 2;
  }
  const uint32_t seed = (uint32_t)atoi(argv[1]);
  const int32_t batch = atoi(argv[2]);
  const int64_t rounds = atoll(argv[3]);
  clrrt_adapter::MotionPlanner::Config cfg;
  const double goal0[4] = {0, 0, 0, 0};
  clrrt_params_default(&cfg.base, 0.0, goal0, 5.0);
  cfg.base.collision_mode = CLRRT_COLLISION_OBB;
  cfg.cap.max_nodes = 1 << 16;
  cfg.cap.max_rows = 1 << 21;
  cfg.cap.max_batch = batch;
  cfg.cap.max_obstacles = 16;
  cfg.commit_path = true;
  cfg.carry_tree = atoi(argv[4]) != 0;
  cfg.mode = CLRRT_MODE_BATCH;
  cfg.batch = batch;
  cfg.n_iters = batch * rounds;
  // the car's world state at the three queries, and the fixed world goal
  const double states[3][6] = {{0.0, 0.0, 0.0, 0.0, 1.0, 0.0}, {0.3, 0.01, 0.01, 0.0, 1.5, 0.0}, {0.7, 0.03, 0.02, 0.0, 2.0, 0.0}};
  const double goal_w[4] = {40.0, 0.0, 0.0, 0.0};
  try {
    clrrt_adapter::MotionPlanner mp(cfg, seed);
    for (int q = 0; q < 3; q++) {
      const double* st = states[q];
      mp.updateState(std::vector<double>(st, st + 6));
      mp.updateObstacles(boxes_in_car_frame(st));
      clrrt_adapter::MotionRequest req;
      {  // replan.goal_in_car_frame
        const double c = std::cos(st[2]), s = std::sin(st[2]);
        req.goal[0] = goal_w[0] * c - st[0] * c - st[1] * s + goal_w[1] * s;
        req.goal[1] = goal_w[1] * c - st[1] * c + st[0] * s - goal_w[0] * s;
        req.goal[2] = goal_w[2] - st[2];
        req.goal[3] = goal_w[3];
      }
      req.vmax = 5.0;
      clrrt_adapter::PlanReport rep;
      const bool found = mp.planMotion(req, nullptr, &rep);
      int32_t pn = 0;
      int64_t pr = 0;
      clrrt_adapter::check(mp.ctx(), clrrt_path_size(mp.ctx(), &pn, &pr), "clrrt_path_size");
      std::vector<clrrt_node> nodes((size_t)(pn > 0 ? pn : 1));
      std::vector<double> rows(10 * (size_t)(pr > 0 ? pr : 1));
      if (pn > 0) clrrt_adapter::check(mp.ctx(), clrrt_path_download(mp.ctx(), nodes.data(), rows.data()), "clrrt_path_download");
      printf("query %d found %d outcome %d carried %d subtree %lld collided %lld kept %lld depth %d start %lld tree %lld rows %lld "
             "fnv %016llx path", q, (int)found, rep.reinit_outcome, (int)rep.carried, (long long)rep.rebase.nodes_subtree,
             (long long)rep.rebase.nodes_collided, (long long)rep.rebase.nodes_kept, (int)rep.rebase.depth,
             (long long)rep.start_size, (long long)rep.tree_size, (long long)pr,
             (unsigned long long)fnv1a(rows.data(), 10 * (size_t)pr * sizeof(double)));
      for (int32_t id : rep.path) printf(" %d", id);
      printf("\n");
    }
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
