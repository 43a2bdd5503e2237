// One planMotion query in the occupancy-grid collision mode with the occupancy clearance in the obstacle cost term
// (MotionPlanner::updateOccupancy + setOccupancyClearance of include/clrrt_adapter.hpp), linked against libclrrt (no
// Python): the static world is a wall with a gap, there are no detections, and Wcost[2] = 2 prices the distance to
// the wall.  Prints the clearance record, the tree size, the fail counters, the best path's ids and an FNV-1a of the
// costS bits of every tree node; tests/test_native_occ_clearance.py runs the same query through the Python binding
// and compares.
// Usage: occ_clearance <seed> <batch> <rounds> <clear_max>
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

// The wall of tests/native/occ_plan.cpp: 200 x 96 cells of 0.25 m, corner (-5, -12); columns i0, i0 + 1 occupied where
// the cell centre's y is outside [-3, 3).
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
  if (argc < 5) {
    fprintf(stderr, "usage: %s seed batch rounds clear_max\n", argv[0]);
    return 2;
  }
  const uint32_t seed = (uint32_t)atoi(argv[1]);
  const int32_t batch = atoi(argv[2]);
  const int64_t rounds = atoll(argv[3]);
  const double clear_max = atof(argv[4]);
  clrrt_adapter::MotionPlanner::Config cfg;
  const double goal0[4] = {0, 0, 0, 0};
  clrrt_params_default(&cfg.base, 0.0, goal0, 5.0);
  cfg.base.collision_mode = CLRRT_COLLISION_OCC;
  cfg.base.Wcost[2] = 2.0;
  cfg.cap.max_nodes = 1 << 16;
  cfg.cap.max_rows = 1 << 21;
  cfg.cap.max_batch = batch;
  cfg.cap.max_obstacles = 16;
  cfg.commit_path = true;
  cfg.mode = CLRRT_MODE_BATCH;
  cfg.batch = batch;
  cfg.n_iters = batch * rounds;
  try {
    clrrt_adapter::MotionPlanner mp(cfg, seed);
    mp.updateState({0.0, 0.0, 0.0, 0.0, 1.0, 0.0});
    mp.updateObstacles({});
    mp.updateOccupancy(wall(16.0));
    mp.setOccupancyClearance(clear_max);
    clrrt_adapter::MotionRequest req;
    const double goal[4] = {40.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 4; k++) req.goal[k] = goal[k];
    req.vmax = 5.0;
    clrrt_adapter::PlanReport rep;
    const bool found = mp.planMotion(req, nullptr, &rep);
    clrrt_clearance_info_t ci;
    clrrt_adapter::check(mp.ctx(), clrrt_occupancy_clearance_info(mp.ctx(), &ci), "clrrt_occupancy_clearance_info");
    std::vector<clrrt_node> nodes((size_t)rep.tree_size);
    clrrt_adapter::check(mp.ctx(), clrrt_tree_download(mp.ctx(), 0, rep.tree_size, nodes.data()), "clrrt_tree_download");
    std::vector<float> cost;
    for (const clrrt_node& n : nodes) cost.push_back(n.costS);
    printf("found %d on %d baked %d field_bytes %lld tree %lld counters %lld %lld %lld %lld costS %016llx path", (int)found,
           ci.on, ci.baked, (long long)ci.field_bytes, (long long)rep.tree_size, (long long)rep.counters[0],
           (long long)rep.counters[1], (long long)rep.counters[2], (long long)rep.counters[3],
           (unsigned long long)fnv1a(cost.data(), cost.size() * sizeof(float)));
    for (int32_t id : rep.path) printf(" %d", id);
    printf("\n");
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
