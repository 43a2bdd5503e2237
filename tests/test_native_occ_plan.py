"""planMotion in the occupancy-grid collision mode through the C++ adapter (MotionPlanner::updateOccupancy,
include/clrrt_adapter.hpp) with no Python in the loop (tests/native/occ_plan.cpp): two 5 Hz queries against a wall
with a gap.  The same two queries run through the Python binding's entry points in planMotion's order; the re-init
outcome, tree size, fail counters, committed path ids and the hash of the path's rows must agree."""
import os
import re
import subprocess

import numpy as np
import pytest

import clrrt
from clrrt import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "occ_plan")
SEED, BATCH, ROUNDS = 11, 256, 6
STATES = [(0.0, 0.0, 0.0, 0.0, 1.0, 0.0), (2.0, 0.0, 0.0, 0.0, 2.0, 0.0)]
GOALS = [(40.0, 0.0, 0.0, 0.0), (38.0, 0.0, 0.0, 0.0)]
WALLS = [16.0, 14.0]


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _wall(wall_x):
    """The cells of occ_plan.cpp's wall()."""
    x0, y0, res, w, h = -5.0, -12.0, 0.25, 200, 96
    cells = np.zeros((h, w), np.uint8)
    i0 = int((wall_x - x0) / res + 0.5)
    cy = y0 + (np.arange(h) + 0.5) * res
    cells[(cy < -3.0) | (cy >= 3.0), i0:i0 + 2] = 1
    return x0, y0, res, cells, 0.25


def test_occ_plan_program_compiles():
    """CPU: the adapter with its occupancy entry points and the program compile (host C++ only)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "occ_plan.cpp")], check=True)


@pytest.mark.gpu
def test_native_occ_plan_matches_the_binding():
    assert os.path.exists(EXE), "tests/native/occ_plan not built (make -C cl-rrt_amd/csrc)"
    run = subprocess.run([EXE, str(SEED), str(BATCH), str(ROUNDS)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    got = []
    for line in run.stdout.splitlines():
        m = re.match(r"query (\d+) found (\d) outcome (-?\d+) tree (\d+) occupied (\d+) counters (\d+) (\d+) (\d+) (\d+) "
                     r"rows (\d+) fnv ([0-9a-f]{16}) path(.*)", line)
        if m:
            got.append(dict(found=int(m[2]), outcome=int(m[3]), tree=int(m[4]), occupied=int(m[5]),
                            counters=[int(m[k]) for k in (6, 7, 8, 9)], rows=int(m[10]), fnv=int(m[11], 16),
                            ids=[int(v) for v in m[12].split()]))
    assert len(got) == 2

    base = clrrt.default_params(v0=0.0, goal=(0.0, 0.0, 0.0, 0.0), vmax=5.0, collision_mode=abi.CLRRT_COLLISION_OCC)
    pl = clrrt.Planner(base, max_nodes=1 << 16, max_rows=1 << 21, max_batch=BATCH, max_obstacles=16)
    rng = clrrt.Rng(SEED)
    try:
        for q in range(2):
            st = STATES[q]
            pl.reset_counters()
            p = abi.Params.from_buffer_copy(bytes(base))
            p.ref_res = max(abs(st[4]) * p.ref_int, p.ref_mindist)
            p.vmax = 5.0
            for k in range(4):
                p.goal[k] = GOALS[q][k]
            pl.set_params(p)
            pl.set_obstacles(np.zeros((0, 7)))
            x0, y0, res, cells, inflate = _wall(WALLS[q])
            pl.set_occupancy(x0, y0, res, cells, inflate)
            pl.path_transform(False, st[:3])
            oc = pl.tree_init_from_path([0.0, 0.0, 0.0, st[3], st[4], st[5]])
            pl.expand(rng, n_iters=BATCH * ROUNDS, mode=clrrt.CLRRT_MODE_BATCH, batch=BATCH)
            tree = pl.size()[0]
            ids, _, _ = pl.extract_best_path()
            pl.path_commit(ids)
            pl.path_transform(True, st[:3])
            _, rows = pl.path_download()
            c = pl.counters()
            want = dict(found=int(len(ids) > 0), outcome=oc, tree=tree, occupied=int(cells.sum()),
                        counters=[c["sim_count"], c["fail_collision"], c["fail_acclimit"], c["fail_iterlimit"]],
                        rows=len(rows), fnv=_fnv1a(np.ascontiguousarray(rows).tobytes()), ids=ids)
            assert got[q] == want, (q, got[q], want)
            # the wall takes part: rollouts fail on it, and the committed path goes through the gap
            assert want["found"] and len(rows) > 10 and (q > 0 or c["fail_collision"] > 0)
        assert got[1]["outcome"] == abi.REINIT_KEPT  # the second query starts from the first one's path
    finally:
        pl.close()
