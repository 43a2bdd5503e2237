"""planMotion with the occupancy clearance in the obstacle cost term through the C++ adapter
(MotionPlanner::updateOccupancy + setOccupancyClearance, include/clrrt_adapter.hpp) with no Python in the loop
(tests/native/occ_clearance.cpp): one query against a wall with a gap, Wcost[2] = 2.  The same query runs through the
Python binding's entry points in planMotion's order; the clearance record, tree size, fail counters, best path ids and
the hash of every node's costS bits must agree."""
import os
import re
import subprocess

import numpy as np
import pytest

import clrrt
from clrrt import abi
from test_native_occ_plan import _fnv1a, _wall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "occ_clearance")
SEED, BATCH, ROUNDS, CLEAR_MAX = 11, 256, 6, 3.0


def test_occ_clearance_program_compiles():
    """CPU: the adapter with setOccupancyClearance and the program compile (host C++ only)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "occ_clearance.cpp")], check=True)


def _plan(clear_max):
    base = clrrt.default_params(v0=0.0, goal=(0.0, 0.0, 0.0, 0.0), vmax=5.0, collision_mode=abi.CLRRT_COLLISION_OCC)
    base.Wcost[2] = 2.0
    pl = clrrt.Planner(base, max_nodes=1 << 16, max_rows=1 << 21, max_batch=BATCH, max_obstacles=16)
    try:
        st = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        pl.reset_counters()
        p = abi.Params.from_buffer_copy(bytes(base))
        p.ref_res = max(abs(st[4]) * p.ref_int, p.ref_mindist)
        p.vmax = 5.0
        for k, v in enumerate((40.0, 0.0, 0.0, 0.0)):
            p.goal[k] = v
        pl.set_params(p)
        pl.set_obstacles(np.zeros((0, 7)))
        x0, y0, res, cells, inflate = _wall(16.0)
        pl.set_occupancy(x0, y0, res, cells, inflate)
        pl.set_occupancy_clearance(clear_max)
        pl.path_transform(False, st[:3])
        pl.tree_init_from_path([0.0, 0.0, 0.0, st[3], st[4], st[5]])
        pl.expand(clrrt.Rng(SEED), n_iters=BATCH * ROUNDS, mode=clrrt.CLRRT_MODE_BATCH, batch=BATCH)
        tree = pl.size()[0]
        ids, _, _ = pl.extract_best_path()
        c = pl.counters()
        ci = pl.occupancy_clearance_info()
        cost = np.ascontiguousarray(pl.nodes()["costS"], dtype=np.float32)
        return dict(found=int(len(ids) > 0), on=ci["on"], baked=ci["baked"], field_bytes=ci["field_bytes"], tree=tree,
                    counters=[c["sim_count"], c["fail_collision"], c["fail_acclimit"], c["fail_iterlimit"]],
                    costS=_fnv1a(cost.tobytes()), ids=list(ids))
    finally:
        pl.close()


@pytest.mark.gpu
def test_native_occ_clearance_matches_the_binding():
    assert os.path.exists(EXE), "tests/native/occ_clearance not built (make -C cl-rrt_amd/csrc)"
    run = subprocess.run([EXE, str(SEED), str(BATCH), str(ROUNDS), str(CLEAR_MAX)], capture_output=True, text=True,
                         timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.match(r"found (\d) on (\d) baked (\d) field_bytes (\d+) tree (\d+) counters (\d+) (\d+) (\d+) (\d+) "
                 r"costS ([0-9a-f]{16}) path(.*)", run.stdout.strip().splitlines()[-1])
    assert m, run.stdout
    got = dict(found=int(m[1]), on=int(m[2]), baked=int(m[3]), field_bytes=int(m[4]), tree=int(m[5]),
               counters=[int(m[k]) for k in (6, 7, 8, 9)], costS=int(m[10], 16), ids=[int(v) for v in m[11].split()])
    want = _plan(CLEAR_MAX)
    assert got == want, (got, want)
    assert want["found"] and want["on"] == 1 and want["baked"] == 1 and want["field_bytes"] == 4 * 200 * 96
    # the clearance takes part: the same query with it off grows the same tree with other costs
    off = _plan(0.0)
    assert (off["tree"], off["counters"]) == (want["tree"], want["counters"]) and off["costS"] != want["costS"]
    assert off["on"] == 0 and off["baked"] == 0 and off["field_bytes"] == 0
