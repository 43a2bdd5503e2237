"""The root seed's effect on the walk search's work (option nn_root_seed, clrrt_nnwalk.hip): on cfg3 trees grown to
argv[1:] million nodes (default 1.2 2.8), searches the explore and the optimize samples of a fresh 16384-sample
round with the seed off and on and prints, per kind: the search time, tiles visited and exact keys per sample,
overflow records, and the seed's two counters (clrrt_debug_counters 27: optimize samples whose final list is the
seeded list; 63: optimize samples seeded with fewer than 11 entries).  The lists of both settings are compared."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
import torch  # noqa: E402,F401
import clrrt  # noqa: E402
from clrrt import abi, scenes  # noqa: E402

targets = [float(x) for x in sys.argv[1:]] or [1.2, 2.8]
cap = int(max(targets) * 1e6) + (1 << 20)
pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=cap,
                   max_rows=min(1 << 31, cap * 72), max_batch=16384)
pl.set_obstacles(scenes.urban_scene(200))
pl.tree_init()
rng = clrrt.Rng(5)
smp = clrrt.Rng(77).draw_samples(pl.params, 16384)
kinds = (("mixed", list(smp)), ("explore", [s for s in smp if s.explore]), ("optimize", [s for s in smp if not s.explore]))
for tgt in targets:
    while pl.size()[0] < tgt * 1e6:  # fixed-count rounds: the same tree on every build
        if pl.expand(rng, n_iters=16 * 16384, mode=clrrt.CLRRT_MODE_BATCH, batch=16384)["capacity_stop"]:
            break
    print(f"{pl.size()[0] / 1e6:6.2f} M nodes", flush=True)
    for lab, sub in kinds:
        lists = []
        for seed in (0, 1):
            pl.set_option("nn_root_seed", seed)
            pl.sort_nodes_batch(sub, exact=False)  # warm: the index of this tree and setting
            best = 1e9
            for _ in range(3):
                pl.reset_counters()  # the counters below are those of the last repetition
                t0 = time.perf_counter()
                got = pl.sort_nodes_batch(sub, exact=False)
                best = min(best, time.perf_counter() - t0)
            lists.append(got)
            w, d = pl.search_work(), pl.debug_counters()
            ns = max(1, w["samples"])
            print(f"   {lab:8s} {len(sub):5d} samples, nn_root_seed {seed}: {best * 1e3:7.2f} ms; tiles/sample "
                  f"{w['tiles'] / ns:6.0f}, exact keys/sample {w['exact_keys'] / ns:6.0f}, overflow records {d[32]}; "
                  f"final list = seeded list {d[27]}, seeded short {d[63]}", flush=True)
        same = np.array_equal(lists[0][0], lists[1][0]) and np.array_equal(lists[0][1].view(np.uint32),
                                                                          lists[1][1].view(np.uint32))
        print(f"   {lab:8s} lists equal: {same}", flush=True)
        if not same:
            sys.exit(1)
