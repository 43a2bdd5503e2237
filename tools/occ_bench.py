#!/usr/bin/env python3
"""Occupancy-grid collision mode against the obstacle list on the cfg3 scene (200 static boxes): 16384 samples per
round, 8 rounds, deferred samples as bench.py runs cfg3 (defer_steps 128).

  mode 1   the boxes as CLRRT_COLLISION_OBB takes them (run it against another build with CLRRT_LIB=... to compare
           two commits -- or, where the other build's binding differs too, with CLRRT_PKG=<its cl-rrt_amd
           directory>: the mode-1 figures are what a change must leave alone)
  mode 2   the same boxes rasterised at res 0.2 (scenes.rasterize), no obstacle list, CLRRT_COLLISION_OCC

Per run: rollout-kernel ms per launch (clrrt_kernel_time family 1), the share of simulated steps that took the
grid's exact scan (raw work counter 3 over work counter 0), nodes grown.  Then the bake time of 512 x 512 and
2048 x 2048 grids (2 % random fill; clrrt_occupancy_info).  Writes a text summary (default profiles/occ_grid.txt).

  mode 2g  mode 2 with Wcost[2] = 2 (the gap-value instantiation of the rollout kernels), clearance off
  mode 2gc the same with the occupancy clearance on (clrrt_set_occupancy_clearance, clear_max 3): the difference to
           2g is the distance-field lookups
With 2gc among the modes, the field bake time (clrrt_occupancy_clearance_info) of 512 x 512 and 2048 x 2048 grids at
1 % random fill and with a single occupied cell follows.

  mode 2L4 / 2L8  the static scene plus the 20 movers of urban_scene(200, 20), rasterised into 4 / 8 layers of 0.5 s
           from t = 0 (scenes.rasterize_layers, clrrt_set_occupancy_layers), no obstacle list
  mode 2m  that scene with the static boxes as the single grid and the 20 movers as boxes of the obstacle list: the
           like-for-like cost of cells against boxes for 2L4
With 2L8 among the modes, the bake time of stacks of 512 x 512 x 8 and 2048 x 512 x 16 (2 % fill) follows.

  python tools/occ_bench.py [--runs 3] [--modes 1,2,2g,2gc,2L4,2L8,2m] [--out profiles/occ_grid.txt] [--label text]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("CLRRT_PKG") or os.path.join(ROOT, "cl-rrt_amd"))  # CLRRT_PKG: another build's tree

import clrrt  # noqa: E402
from clrrt import abi, scenes  # noqa: E402

B, ROUNDS, DEFER = 16384, 8, 128
GRID = dict(x0=0.0, y0=-26.0, res=0.2, w=330, h=260)


LAYER_T0, LAYER_DT = 0.0, 0.5
PLACES = {1: "LDS", 2: "global memory", 3: "global memory, the union reach map in LDS"}


def grow(mode, obs, cells, w2=0.0, clear_max=0.0):
    params = clrrt.default_params(collision_mode=mode)
    params.Wcost[2] = w2
    pl = clrrt.Planner(params, max_nodes=1 << 20, max_rows=1 << 26, max_batch=B, max_obstacles=max(1, len(obs)))
    try:
        pl.set_option("defer_steps", DEFER)
        pl.set_obstacles(obs)
        if cells is not None and cells.ndim == 3:
            pl.set_occupancy_layers(GRID["x0"], GRID["y0"], GRID["res"], cells, LAYER_T0, LAYER_DT)
        elif cells is not None:
            pl.set_occupancy(GRID["x0"], GRID["y0"], GRID["res"], cells)
        if clear_max:
            pl.set_occupancy_clearance(clear_max)
        pl.enable_timing(True)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(1), n_iters=B * ROUNDS, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
        ms, launches = pl.kernel_time(1)
        d = pl.debug_counters()
        info = pl.occupancy_info() if cells is not None else None
        return dict(ms_per_launch=ms / max(1, launches), launches=launches, steps=d[0], scans=d[3],
                    nodes=pl.size()[0], rounds=st["rounds"], info=info)
    finally:
        pl.close()


def bake(n, runs):
    cells = (np.random.default_rng(n).random((n, n)) < 0.02).astype(np.uint8)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OCC), max_nodes=1 << 10,
                       max_rows=1 << 14, max_batch=64)
    try:
        out = []
        for _ in range(runs + 1):  # the first call allocates
            pl.set_occupancy(-0.05 * n, -0.05 * n, 0.1, cells)
            out.append(pl.occupancy_info())
        return out[1:]
    finally:
        pl.close()


def bake_stack(w, h, layers, runs):
    cells = (np.random.default_rng(w + layers).random((layers, h, w)) < 0.02).astype(np.uint8)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OCC), max_nodes=1 << 10,
                       max_rows=1 << 14, max_batch=64)
    try:
        out = []
        for _ in range(runs + 1):  # the first call allocates
            pl.set_occupancy_layers(-0.05 * w, -0.05 * h, 0.1, cells, LAYER_T0, LAYER_DT)
            out.append(pl.occupancy_layers_info())
        return out[1:]
    finally:
        pl.close()


def field_bake(n, single, runs):
    if single:
        cells = np.zeros((n, n), np.uint8)
        cells[n // 3, n // 5] = 1
    else:
        cells = (np.random.default_rng(n).random((n, n)) < 0.01).astype(np.uint8)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OCC), max_nodes=1 << 10,
                       max_rows=1 << 14, max_batch=64)
    try:
        pl.set_occupancy_clearance(3.0)
        out = []
        for _ in range(runs + 1):  # the first call allocates
            pl.set_occupancy(-0.05 * n, -0.05 * n, 0.1, cells)
            out.append((pl.occupancy_clearance_info()["bake_ms"], pl.occupancy_info()["bake_ms"]))
        return out[1:]
    finally:
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_grid.txt"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    obs = scenes.urban_scene(200)
    lines = [f"occ_bench {args.label}: cfg3 scene (200 static boxes), {B} samples x {ROUNDS} rounds, defer_steps {DEFER}; "
             f"library {os.path.relpath(clrrt.LIB_PATH, ROOT)}"]
    layered = hasattr(clrrt.Planner, "set_occupancy_layers")
    for name in (m for m in args.modes.split(",") if m):
        mode = int(name[0])
        if mode == 2 and not hasattr(abi, "CLRRT_COLLISION_OCC"):
            continue
        if name == "2gc" and not hasattr(clrrt.Planner, "set_occupancy_clearance"):
            continue
        if name.startswith("2L") and not layered:
            continue
        cells = scenes.rasterize(obs, **GRID) if mode == 2 else None
        boxes = obs if mode == 1 else obs[:0]
        if name.startswith("2L"):
            cells = scenes.rasterize_layers(scenes.urban_scene(200, 20), layers=int(name[2:]), t0=LAYER_T0, dt=LAYER_DT,
                                            **GRID)
        elif name == "2m":
            boxes = scenes.urban_scene(200, 20)[200:]
        res = [grow(mode, boxes, cells, 2.0 if "g" in name else 0.0, 3.0 if name == "2gc" else 0.0)
               for _ in range(args.runs)]
        ms = [r["ms_per_launch"] for r in res]
        lines.append(f"mode {name}: rollout kernel ms per launch {' '.join('%.3f' % v for v in ms)} (spread "
                     f"{(max(ms) - min(ms)) / min(ms) * 100:.1f} %), launches {res[0]['launches']}, nodes "
                     f"{res[0]['nodes']}, steps {res[0]['steps']}")
        if name == "2":
            r = res[0]
            lines.append(f"mode 2: grid {GRID['w']} x {GRID['h']} at res {GRID['res']}, {r['info']['occupied']} occupied "
                         f"cells, maps {r['info']['map_bytes']} B in "
                         f"{PLACES[r['info']['placement']]}; exact scans "
                         f"{r['scans']} of {r['steps']} steps ({100.0 * r['scans'] / max(1, r['steps']):.2f} %)")
        if name.startswith("2L") or name == "2m":
            r = res[0]
            lines.append(f"mode {name}: {r['info']['occupied']} occupied cells in all layers, maps "
                         f"{r['info']['map_bytes']} B in {PLACES[r['info']['placement']]}; exact scans {r['scans']} of "
                         f"{r['steps']} steps ({100.0 * r['scans'] / max(1, r['steps']):.2f} %)")
    if "2L8" in args.modes.split(",") and layered:
        for w, h, layers in ((512, 512, 8), (2048, 512, 16)):
            b = bake_stack(w, h, layers, args.runs)
            lines.append(f"stack bake {w} x {h} x {layers} (2 % fill, maps {b[0]['map_bytes']} B, union reach map "
                         f"{b[0]['union_reach_bytes']} B, {PLACES[b[0]['placement']]}): "
                         f"{' '.join('%.3f' % v['bake_ms'] for v in b)} ms (upload + kernels)")
    if "2" in args.modes.split(","):
        for n in (512, 2048):
            b = bake(n, args.runs)
            lines.append(f"bake {n} x {n} (2 % fill, {b[0]['occupied']} occupied, reach map {b[0]['reach_w']} x "
                         f"{b[0]['reach_h']}): {' '.join('%.3f' % v['bake_ms'] for v in b)} ms (upload + kernels)")
    if "2gc" in args.modes.split(",") and hasattr(clrrt.Planner, "set_occupancy_clearance"):
        for n in (512, 2048):
            for single in (False, True):
                b = field_bake(n, single, args.runs)
                lines.append(f"field bake {n} x {n} ({'one occupied cell' if single else '1 % fill'}): "
                             f"{' '.join('%.3f' % v[0] for v in b)} ms (kernels), beside the map bake's "
                             f"{' '.join('%.3f' % v[1] for v in b)} ms (upload + kernels)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
