// planMotion with a stack of time layers (OccupancyGrid::layers > 1 -> clrrt_set_occupancy_layers) through
// include/clrrt_adapter.hpp's MotionPlanner, linked against libclrrt (no Python).  One query each, same seed:
//   single : the wall with a gap as a single grid;
//   same4  : a stack of 4 layers, each that grid -- the MPC message must be the single grid's byte for byte;
//   gate   : a stack of 8 layers of 0.5 s from t0 = 0.25 s, the gap open in layers 0..3 and filled from layer 4 on -- the
//            query completes and no row of the committed path collides (clrrt_obstacle_distance != 0 for each, every
//            row against the layer of its own time).
// Prints one line per query; tests/test_native_occ_layers.py reads them.
// Usage: occ_layers_plan <seed> <batch> <rounds>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/clrrt_adapter.hpp"

// A grid of 160 x 96 cells of 0.25 m with its corner at (0, -12): the wall's two columns at x = 16, occupied where the
// cell centre's y is outside [-3, 3) -- or everywhere (filled).
static void wall(std::vector<uint8_t>& cells, size_t at, int w, int h, bool filled) {
  const double y0 = -12.0, res = 0.25;
  const int i0 = (int)(16.0 / res + 0.5);
  for (int j = 0; j < h; j++) {
    const double cy = y0 + (j + 0.5) * res;
    if (filled || cy < -3.0 || cy >= 3.0) cells[at + (size_t)j * w + i0] = cells[at + (size_t)j * w + i0 + 1] = 1;
  }
}

static clrrt_adapter::OccupancyGrid stack(int layers, int filled_from) {
  clrrt_adapter::OccupancyGrid g;
  g.dims.x0 = 0.0; g.dims.y0 = -12.0; g.dims.res = 0.25; g.dims.inflate = 0.25;
  g.dims.w = 160; g.dims.h = 96;
  g.layers = layers;
  g.t0 = 0.25; g.dt = 0.5;
  const size_t n = (size_t)g.dims.w * g.dims.h;
  g.cells.assign(n * layers, 0);
  for (int k = 0; k < layers; k++) wall(g.cells, n * k, g.dims.w, g.dims.h, k >= filled_from);
  return g;
}

static void append(std::vector<unsigned char>& b, const std::vector<double>& v) {
  const uint64_t n = v.size();
  const unsigned char* p = (const unsigned char*)&n;
  b.insert(b.end(), p, p + sizeof(n));
  p = (const unsigned char*)v.data();
  b.insert(b.end(), p, p + v.size() * sizeof(double));
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
  clrrt_params_default(&cfg.base, 7.0, goal0, 10.0);
  cfg.base.collision_mode = CLRRT_COLLISION_OCC;
  cfg.cap.max_nodes = 1 << 16;
  cfg.cap.max_rows = 1 << 21;
  cfg.cap.max_batch = batch;
  cfg.cap.max_obstacles = 16;
  cfg.commit_path = true;
  cfg.mode = CLRRT_MODE_BATCH;
  cfg.batch = batch;
  cfg.n_iters = batch * rounds;
  const char* names[3] = {"single", "same4", "gate"};
  std::vector<unsigned char> msgs[3];
  try {
    for (int q = 0; q < 3; q++) {
      clrrt_adapter::MotionPlanner mp(cfg, seed);
      mp.updateState({0.0, 0.0, 0.0, 0.0, 7.0, 0.0});  // world frame = car frame: the path's rows keep the rollouts' clock
      mp.updateObstacles({});
      mp.updateOccupancy(q == 0 ? stack(1, 1) : q == 1 ? stack(4, 4) : stack(8, 4));
      clrrt_adapter::MotionRequest req;
      req.goal[0] = 40.0;
      req.vmax = 10.0;
      clrrt_adapter::MPCTrajectory msg;
      clrrt_adapter::PlanReport rep;
      const bool found = mp.planMotion(req, &msg, &rep);
      for (const auto* v : {&msg.x, &msg.y, &msg.theta, &msg.v, &msg.a, &msg.a_cmd, &msg.d_cmd}) append(msgs[q], *v);
      clrrt_occupancy_layers_info_t li;
      clrrt_adapter::check(mp.ctx(), clrrt_occupancy_layers_info(mp.ctx(), &li), "clrrt_occupancy_layers_info");
      int32_t pn = 0;
      int64_t pr = 0;
      clrrt_adapter::check(mp.ctx(), clrrt_path_size(mp.ctx(), &pn, &pr), "clrrt_path_size");
      std::vector<clrrt_node> nodes((size_t)(pn > 0 ? pn : 1));
      std::vector<double> rows(10 * (size_t)(pr > 0 ? pr : 1)), dist((size_t)(pr > 0 ? pr : 1), -1.0);
      int64_t zero = 0;
      double tmax = 0.0;
      if (pn > 0) {
        clrrt_adapter::check(mp.ctx(), clrrt_path_download(mp.ctx(), nodes.data(), rows.data()), "clrrt_path_download");
        clrrt_adapter::check(mp.ctx(), clrrt_obstacle_distance(mp.ctx(), rows.data(), (int32_t)pr, dist.data()),
                             "clrrt_obstacle_distance");
        for (int64_t i = 0; i < pr; i++) {
          zero += dist[(size_t)i] == 0.0;
          if (rows[10 * (size_t)i + 6] > tmax) tmax = rows[10 * (size_t)i + 6];
        }
      }
      printf("query %s found %d layers %d tree %lld collisions %lld msg %zu rows %lld colliding %lld tmax %.3f same %d\n",
             names[q], (int)found, li.layers, (long long)rep.tree_size, (long long)rep.counters[1], msg.x.size(),
             (long long)pr, (long long)zero, tmax,
             (int)(msgs[q].size() == msgs[0].size() && memcmp(msgs[q].data(), msgs[0].data(), msgs[0].size()) == 0));
    }
  } catch (const std::exception& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
