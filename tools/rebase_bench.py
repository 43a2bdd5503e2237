#!/usr/bin/env python3
"""clrrt_tree_rebase: what carrying the tree across replanning queries costs and what it buys.

  time     device_ms and wall time of Planner.tree_rebase on a tree of the size a cfg5 query ends with (one 200 ms
           BATCH query, 16384 samples per round) and on one of ~2.4 M nodes, with 200 static + 20 moving boxes (mode 1)
           and with the static boxes rasterised into a 512 x 512 grid (mode 2, the movers stay boxes).  Rebasing at node
           0 with the identity pose keeps every node, so it repeats on one tree (the worst case: the whole tree is
           checked, re-costed and moved); then one rebase at the depth-1 node with the most descendants, 0.2 s on.
           Beside it: the time the same run's expansion needed per kept node (its nodes/s) -- the time regrowing them
           would take, which is what says whether carrying pays.
  check    achieved bytes/s of k_rebase_check (clrrt_kernel_time family 6) against rows x 80 B.
  quality  over 5 seeds of the cfg5 scenario, 3 queries of 200 ms each: best-path cost and goal-node count of the last
           query with and without carry_tree (reported, not gated).

Writes a text summary (default profiles/rebase.txt).

  python tools/rebase_bench.py [--runs 3] [--parts time,quality] [--big 2400000] [--out profiles/rebase.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))

import clrrt  # noqa: E402
from clrrt import abi, replan, scenes  # noqa: E402

B, DEFER = 16384, 128
GRID = dict(x0=-20.0, y0=-51.2, res=0.2, w=512, h=512)


def planner(mode, obs, cells):
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 22, max_rows=1 << 28, max_batch=B,
                       max_obstacles=max(1, len(obs)))
    pl.set_option("defer_steps", DEFER)
    pl.set_obstacles(obs)
    if cells is not None:
        pl.set_occupancy(GRID["x0"], GRID["y0"], GRID["res"], cells)
    return pl


def grow(pl, target):
    """One 200 ms query (target None) or rounds until the tree has `target` nodes; (nodes, rows, nodes per second)."""
    pl.tree_init()
    rng = clrrt.Rng(1)
    t0 = time.perf_counter()
    if target is None:
        pl.expand(rng, n_iters=0, budget_ms=200.0, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
    else:
        while pl.size()[0] < target:
            pl.expand(rng, n_iters=B * 8, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
    dt = time.perf_counter() - t0
    n, r = pl.size()
    return n, r, n / dt


def biggest_child(parent):
    """The depth-1 node with the most descendants: every node climbs until its parent is node 0."""
    parent = parent.astype(np.int64)
    top = np.arange(len(parent))
    while True:
        p = parent[top]
        move = p > 0
        if not move.any():
            break
        top = np.where(move, p, top)
    cnt = np.bincount(top[1:], minlength=len(parent))
    return int(np.argmax(cnt)), int(cnt.max()) - 1


def time_part(lines, runs, big):
    obs = scenes.urban_scene(200, 20)
    for label, mode, o, cells in (("mode 1, 200 + 20 boxes", abi.CLRRT_COLLISION_OBB, obs, None),
                                  ("mode 2, 512 x 512 grid + 20 boxes", abi.CLRRT_COLLISION_OCC, obs[200:],
                                   scenes.rasterize(obs[:200], **GRID))):
        for target in (None, big):
            pl = planner(mode, o, cells)
            try:
                n, r, nps = grow(pl, target)
                pl.enable_timing(True)
                res = []
                for _ in range(runs):
                    t0 = time.perf_counter()
                    info = pl.tree_rebase(0, (0.0, 0.0, 0.0), 0.0)
                    res.append((info["device_ms"], (time.perf_counter() - t0) * 1e3, info))
                ck_ms, ck_n = pl.kernel_time(6)
                rows = res[0][2]["rows_before"]
                lines.append(f"{label}, tree {n} nodes / {r} rows (grown at {nps / 1e6:.3f} M nodes/s): rebase of the "
                             f"whole tree, device ms {' '.join('%.3f' % v[0] for v in res)}, wall ms "
                             f"{' '.join('%.3f' % v[1] for v in res)}, kept {res[-1][2]['nodes_kept']} nodes, depth "
                             f"{res[-1][2]['depth']}; regrowing them at the run's rate: "
                             f"{res[-1][2]['nodes_kept'] / nps * 1e3:.1f} ms")
                lines.append(f"    k_rebase_check: {ck_ms / max(1, ck_n):.3f} ms per launch over {rows} rows = "
                             f"{rows * 80 / max(1e-9, ck_ms / max(1, ck_n)) / 1e6:.1f} GB/s of rows x 80 B")
                root, cnt = biggest_child(pl.nodes()["parent"])
                nd = pl.nodes_raw(root, 1)[0]
                x, y, th = nd.state[0], nd.state[1], nd.state[2]
                t0 = time.perf_counter()
                info = pl.tree_rebase(root, (x - 0.5 * np.cos(th), y - 0.5 * np.sin(th), th), nd.state[6])
                lines.append(f"    rebase at depth-1 node {root} ({cnt} descendants): device ms {info['device_ms']:.3f}, "
                             f"wall ms {(time.perf_counter() - t0) * 1e3:.3f}, outcome {info['outcome']}, subtree "
                             f"{info['nodes_subtree']}, collided {info['nodes_collided']}, kept {info['nodes_kept']} "
                             f"nodes / {info['rows_kept']} rows; regrowing them: {info['nodes_kept'] / nps * 1e3:.1f} ms")
            finally:
                pl.close()


def quality_part(lines, seeds=5, queries=3):
    obs = scenes.urban_scene(200, 20)
    mode = abi.CLRRT_COLLISION_OBB
    for carry in (False, True):
        costs, goals, starts = [], [], []
        for seed in range(1, seeds + 1):
            pl = planner(mode, obs, None)
            try:
                be = replan.PlannerBackend(pl, replan.default_make_params(mode), carry_tree=carry)
                rng = clrrt.Rng(seed)
                last = {}

                def expand(q):
                    last["start"] = pl.size()[0]
                    pl.expand(rng, n_iters=0, budget_ms=200.0, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
                    _, last["cost"], last["goal"] = pl.extract_best_path()

                replan.run_queries(be, expand, queries, obs, v0=1.0)
                costs.append(last["cost"]); goals.append(last["goal"]); starts.append(last["start"])
            finally:
                pl.close()
        lines.append(f"cfg5 scenario, query {queries} of {queries}, 200 ms each, carry_tree {carry}: best-path cost "
                     f"{' '.join('%.2f' % c for c in costs)}; goal nodes {' '.join(str(g) for g in goals)}; tree at the "
                     f"query's start {' '.join(str(s) for s in starts)} nodes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parts", default="time,quality")
    ap.add_argument("--big", type=int, default=2400000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebase.txt"))
    args = ap.parse_args()
    lines = [f"rebase_bench: {B} samples per round, defer_steps {DEFER}; library {os.path.relpath(clrrt.LIB_PATH, ROOT)}"]
    parts = args.parts.split(",")
    if "time" in parts:
        time_part(lines, args.runs, args.big)
    if "quality" in parts:
        quality_part(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
