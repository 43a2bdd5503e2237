"""How deep into the root pose's copies an optimize sample's list reaches (CPU oracle; justifies the root roster's K,
clrrt_nnwalk.hip).  Grows the cfg3 scene by BATCH rounds (seed 31, 16384 samples per round, defer_steps 128), draws
fresh samples and takes their lists from the oracle's stable sort.  The copies of the root pose (the root and the nodes
equal to it in x, y, heading and costE) share one optimize key per sample and order by id, so an optimize list is
mostly their first feasible members: the rank by id, within the class, of a list's last member is the roster length
that list needs.  Usage: python tools/root_seed_depth.py [rounds [samples]] > profiles/<name>.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clrrt import abi, scenes  # noqa: E402
from oracle_binding import Oracle  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n_smp = int(sys.argv[2]) if len(sys.argv) > 2 else 1200
B = 16384
o = Oracle(abi.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), scenes.urban_scene(200))
Oracle.srand(31)
o.init_tree()
o.expand_batch(rounds * B, B, stable=True, defer_steps=128, threads=min(32, os.cpu_count() or 4))
t = o.nodes()
N = len(t["parent"])
st, ce = t["state"], t["costE"]
cls = np.nonzero((st[:, 0] == st[0, 0]) & (st[:, 1] == st[0, 1]) & (st[:, 2] == st[0, 2]) & (ce == ce[0]))[0]
rank = np.full(N, -1)
rank[cls] = np.arange(len(cls))  # rank by id within the root class
print(f"cfg3 scene, seed 31, B = {B}, defer_steps 128, {rounds} rounds: {N} nodes, root class {len(cls)} members "
      f"(ids up to {cls[-1]}; {np.count_nonzero(cls < 16384)} below 16384)")
# (pose, costE, ref.back(), ang_par) duplicates: records a search could drop
full = np.concatenate([st[:, :3], ce[:, None].astype(np.float64), t["ref_back"], t["ang_par"][:, None]], axis=1)
print(f"nodes equal to another in all of (pose, costE, ref.back(), ang_par): {N - len(np.unique(full, axis=0))}")
xy, ex = o.draw_samples(n_smp)
for kind in (0, 1):
    sel = np.nonzero(ex == kind)[0]
    last, with_root, only_root = [], 0, 0
    for j in sel:
        ids, _ = o.sort_nodes(xy[j, 0], xy[j, 1], kind, stable=True)
        ids = np.array(ids[:11], dtype=np.int64)
        r = rank[ids]
        with_root += bool((r >= 0).any())
        if len(ids) and (r >= 0).all():
            only_root += 1
            last.append(r.max() + 1)
    name = "explore" if kind else "optimize"
    line = f"{name}: {len(sel)} lists, {with_root} contain a root-pose node, {only_root} consist of the root class only"
    if last:
        p = np.percentile(last, [50, 90, 99])
        line += (f"; rank by id of the last member p50 {p[0]:.0f}, p90 {p[1]:.0f}, p99 {p[2]:.0f}, max {max(last)}; lists "
                 f"within the first 32 / 64 / 256 members: {np.mean(np.array(last) <= 32):.1%} / "
                 f"{np.mean(np.array(last) <= 64):.1%} / {np.mean(np.array(last) <= 256):.1%}")
    print(line, flush=True)
