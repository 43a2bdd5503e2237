"""Work of the lag-2 appended-node search at cfg3 settings (200 obstacles, 16384 samples per round, defer_steps 128):
one 2 s query with option nn_delta_verify, so every appended-node walk (launch_nn_delta_walk) is followed by the brute
force (k_nn_partial) over the same range and caps.  Prints, per sample of a search, what each touched -- the walk's
tiles / records prefiltered / records past the prefilter / exact keys against the brute force's pairs / queued pairs /
exact keys -- and the list comparison (samples compared, differing).  Usage: python3 tools/delta_walk_stats.py [ms]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cl-rrt_amd"))
import clrrt
from clrrt import abi, scenes

B = 16384
ms = float(sys.argv[1]) if len(sys.argv) > 1 else 2000.0
pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=6 << 20, max_rows=(6 << 20) * 64,
                   max_batch=B, max_obstacles=200)
pl.set_option("defer_steps", 128)
pl.set_option("nn_delta_verify", 1)
pl.set_obstacles(scenes.urban_scene(200))
pl.tree_init()
pl.reset_counters()
st = pl.expand(clrrt.Rng(1), n_iters=0, budget_ms=ms, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
d = pl.debug_counters()
sizes = pl.round_sizes()
n = max(1, d[38])
searches = n / B
# a search covers the nodes of two commits
app = [int(sizes[i] - sizes[i - 2]) for i in range(2, len(sizes))]
mean_app = sum(app) / max(1, len(app))
print(f"{st['rounds']} rounds, {pl.size()[0]} nodes; appended-node searches {searches:.0f}, range {mean_app:.0f} nodes "
      f"(two commits, mean); samples compared {d[38]}, differing {d[39]}")
print(f"walk per sample: super-tile visits {d[40] / n:.1f}, tiles {d[41] / n:.1f} = {32 * d[41] / n:.0f} records "
      f"prefiltered ({32 * d[41] / n / max(1, mean_app) * 100:.1f} % of the range), past the prefilter {d[42] / n:.1f}, "
      f"stage-2 dropped {d[52] / n:.1f}, exact keys {d[43] / n:.1f}")
print(f"brute force per sample: pairs {mean_app:.0f}, queued {d[54] / n:.1f}, exact keys {d[55] / n:.1f}")
pl.close()
