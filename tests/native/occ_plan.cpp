// Two 5 Hz planMotion queries in the occupancy-grid collision mode (CLRRT_COLLISION_OCC) through
// include/clrrt_adapter.hpp's MotionPlanner, linked against libclrrt (no Python): the static world is a wall with a
// gap, given per query in the car frame by updateOccupancy; there are no detections.  Prints, per query, the re-init
// outcome, tree size, fail counters, the committed path's ids and an FNV-1a of its rows (world frame);
// tests/test_native_occ_plan.py runs the same two queries through the Python binding and compares.
// Usage: occ_plan <seed> <batch> <rounds>
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

// The wall of the test (tests/test_native_occ_plan.py builds the same cells): a grid of 200 x 96 cells of 0.25 m with
// its corner at (-5, -12); columns i0, i0 + 1 occupied where the cell centre's y is outside [-3, 3).
static clrrt_adapter::OccupancyGrid wall(double wall_x) {
  clrrt_adapter::OccupancyGrid g;
  g.dims.x0 = -5.0; g.dims.y0 = -12.0; g.dims.res = 0.25; g.dims.inflate = 0.25;
  g.dims.w = 200; g.dims.h = 96;
  g.cells.assign((size_t)g.dims.w * g.dims.h, 0);
  const int i0 = (int)((wall_x - g.dims.x0) / g.dims.res + 0.5);
  for (int j = 0; j < g.dims.h; j++) {
    const double cy = g.dims.y0 + (j + 0.5) * g.dims.res;
    if (cy < -3.0 || cy >= 3.0) g.cells[(size_t)j * g.dims.w + i0] = g.cells[(size_t)j * g.dims.w + i0 + 1] = 1;
  }
  return g;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s seed batch rounds\n", argv[0]);
    return 2;
  }
  const uint32_t seed = (uint32_t)atoi(argv[1]);
  const int32_t batch = atoi(argv[2]);
  const int64_t rounds = atoll(argv[3]);
  clrrt_adapter::MotionPlanner::Config cfg;
  const double goal0[4] = {0, 0, 0, 0};
  clrrt_params_default(&cfg.base, 0.0, goal0, 5.0);
  cfg.base.collision_mode = CLRRT_COLLISION_OCC;
  cfg.cap.max_nodes = 1 << 16;
  cfg.cap.max_rows = 1 << 21;
  cfg.cap.max_batch = batch;
  cfg.cap.max_obstacles = 16;
  cfg.commit_path = true;
  cfg.mode = CLRRT_MODE_BATCH;
  cfg.batch = batch;
  cfg.n_iters = batch * rounds;
  // the car's world state and the wall's distance ahead of it at the two queries (the car has moved 2 m)
  const double states[2][6] = {{0.0, 0.0, 0.0, 0.0, 1.0, 0.0}, {2.0, 0.0, 0.0, 0.0, 2.0, 0.0}};
  const double goals[2][4] = {{40.0, 0.0, 0.0, 0.0}, {38.0, 0.0, 0.0, 0.0}};
  const double walls[2] = {16.0, 14.0};
  try {
    clrrt_adapter::MotionPlanner mp(cfg, seed);
    for (int q = 0; q < 2; q++) {
      mp.updateState(std::vector<double>(states[q], states[q] + 6));
      mp.updateObstacles({});
      mp.updateOccupancy(wall(walls[q]));
      clrrt_adapter::MotionRequest req;
      for (int k = 0; k < 4; k++) req.goal[k] = goals[q][k];
      req.vmax = 5.0;
      clrrt_adapter::PlanReport rep;
      const bool found = mp.planMotion(req, nullptr, &rep);
      clrrt_occupancy_info_t info;
      clrrt_adapter::check(mp.ctx(), clrrt_occupancy_info(mp.ctx(), &info), "clrrt_occupancy_info");
      int32_t pn = 0;
      int64_t pr = 0;
      clrrt_adapter::check(mp.ctx(), clrrt_path_size(mp.ctx(), &pn, &pr), "clrrt_path_size");
      std::vector<clrrt_node> nodes((size_t)(pn > 0 ? pn : 1));
      std::vector<double> rows(10 * (size_t)(pr > 0 ? pr : 1));
      if (pn > 0) clrrt_adapter::check(mp.ctx(), clrrt_path_download(mp.ctx(), nodes.data(), rows.data()), "clrrt_path_download");
      printf("query %d found %d outcome %d tree %lld occupied %lld counters %lld %lld %lld %lld rows %lld fnv %016llx path", q,
             (int)found, rep.reinit_outcome, (long long)rep.tree_size, (long long)info.occupied,
             (long long)rep.counters[0], (long long)rep.counters[1], (long long)rep.counters[2],
             (long long)rep.counters[3], (long long)pr,
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
