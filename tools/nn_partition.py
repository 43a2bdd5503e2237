"""Cost of the tree-partitioned nearest-node search (clrrt_nn_range + clrrt_nn_merge) on large trees.

Grows the cfg3 scene by BATCH expansion as tools/nn_large.py does and, at each target size (millions of nodes,
argv[1:]; a size beyond the capacity stops at the capacity), searches one fresh 16384-sample round over the W
contiguous node ranges of clrrt.dist.node_range for W in {1, 2, 4, 8}.  Per partition it prints

  * the index build: the first search of the range (which builds the range's index) minus a repeated one,
    device ms of kernel family 0;
  * the search: device ms of kernel family 3 (the walk search alone) of the repeated search, best of 3;
  * walk tiles visited and exact keys per sample of that search;

and per W the merge kernel's device ms (clrrt_nn_merge over the W list sets, family 0 of that call) and the largest
partition's search against the W = 1 search -- the per-rank search cost of a W-rank partitioned round.  The merged
lists are compared with the W = 1 lists (ids and key bits) as a check.

  python tools/nn_partition.py 2.8 16 > profiles/nn_partition.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
import torch  # noqa: E402,F401
import clrrt  # noqa: E402
from clrrt import abi, scenes  # noqa: E402
from clrrt import dist as cdist  # noqa: E402

G = 16384
targets = [float(x) for x in sys.argv[1:]] or [2.8, 16.0]
cap = int(max(targets) * 1e6) + (1 << 20)
pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=cap,
                   max_rows=min(1 << 31, cap * 72), max_batch=G)
pl.set_obstacles(scenes.urban_scene(200))
pl.tree_init()
for kv in os.environ.get("CLRRT_OPTS", "").split(","):
    if kv:
        k, v = kv.split("=")
        pl.set_option(k, int(v))
rng = clrrt.Rng(5)
smp = clrrt.Rng(77).draw_samples(pl.params, G)
t_grow = time.perf_counter()


def timed(fn):
    """(family 0 ms, family 3 ms, search work) of one call."""
    a0, a3 = pl.kernel_time(0)[0], pl.kernel_time(3)[0]
    pl.reset_counters()
    out = fn()
    return pl.kernel_time(0)[0] - a0, pl.kernel_time(3)[0] - a3, pl.search_work(), out


print(f"# tree-partitioned search of one {G}-sample round: contiguous node-id ranges, W = 1, 2, 4, 8")
for tgt in targets:
    pl.enable_timing(False)
    while pl.size()[0] < tgt * 1e6:  # fixed-count rounds: the same tree on every build
        st = pl.expand(rng, n_iters=16 * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
        if st["capacity_stop"]:
            break
    N = pl.size()[0]
    pl.enable_timing(True)  # device events around the kernel families, for the measured calls only
    print(f"{N / 1e6:6.2f} M nodes (grown in {time.perf_counter() - t_grow:5.1f} s)", flush=True)
    whole, t_whole = None, None
    for W in (1, 2, 4, 8):
        parts, worst = [], 0.0
        for r in range(W):
            first, count = cdist.node_range(N, W, r)
            f0, _, _, _ = timed(lambda: pl.nn_range(smp, first, count))  # builds the range's index
            best = None
            for _ in range(3):
                g0, g3, w, lists = timed(lambda: pl.nn_range(smp, first, count))
                if best is None or g3 < best[1]:
                    best = (g0, g3, w)
            g0, g3, w = best
            parts.append(lists)
            worst = max(worst, g3)
            print(f"   W={W} part {r}: nodes [{first}, {first + count}): index build {max(0.0, f0 - g0):7.2f} ms, search "
                  f"{g3:7.2f} ms, tiles/sample {w['tiles'] / G:7.1f}, exact keys/sample {w['exact_keys'] / G:7.1f}",
                  flush=True)
        stack = [np.stack([q[i] for q in parts]) for i in range(3)]
        m0 = min(timed(lambda: pl.nn_merge(*stack))[0] for _ in range(3))
        merged = pl.nn_merge(*stack)
        if W == 1:
            whole, t_whole = merged, worst
        same = (np.array_equal(merged[0], whole[0]) and np.array_equal(merged[2], whole[2]) and
                np.array_equal(merged[1].view(np.uint32), whole[1].view(np.uint32)))
        print(f"   W={W}: merge kernel {m0:6.3f} ms ({W} x {G} lists, {W * G * 84 / 1e6:.2f} MB gathered per round); slowest "
              f"partition's search {worst:7.2f} ms = {worst / t_whole:.2f} x the W=1 search (1/W = {1 / W:.3f}); merged "
              f"lists {'equal' if same else 'DIFFER from'} the W=1 lists", flush=True)
pl.close()
