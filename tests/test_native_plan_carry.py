"""planMotion with a carried tree through the C++ adapter (MotionPlanner::Config::carry_tree, include/clrrt_adapter.hpp)
with no Python in the loop (tests/native/plan_carry.cpp): three 5 Hz queries among six static boxes.  The same queries
run through the Python binding's replanning backend (replan.PlannerBackend(carry_tree=True)); the re-init outcome, the
rebase counts, the tree sizes, the committed path ids and the hash of the path's rows must agree."""
import os
import re
import subprocess

import numpy as np
import pytest

import clrrt
from clrrt import abi, replan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "plan_carry")
SEED, BATCH, ROUNDS = 11, 256, 4
STATES = [(0.0, 0.0, 0.0, 0.0, 1.0, 0.0), (0.3, 0.01, 0.01, 0.0, 1.5, 0.0), (0.7, 0.03, 0.02, 0.0, 2.0, 0.0)]
GOAL_W = (40.0, 0.0, 0.0, 0.0)
BOXES = np.array([[12.0, 4.5, 0.3, 3.0, 1.5, 0, 0], [18.0, -4.0, -0.2, 2.5, 1.5, 0, 0], [25.0, 3.0, 0.0, 2.0, 2.0, 0, 0],
                  [30.0, -3.5, 0.5, 3.0, 1.0, 0, 0], [8.0, -6.0, 0.0, 4.0, 1.0, 0, 0], [35.0, 6.0, 0.1, 2.0, 2.0, 0, 0]])


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_plan_carry_program_compiles():
    """CPU: the adapter with carry_tree and the program compile (host C++ only)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "plan_carry.cpp")], check=True)


def _native(carry):
    run = subprocess.run([EXE, str(SEED), str(BATCH), str(ROUNDS), str(int(carry))], capture_output=True, text=True,
                         timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    got = []
    for line in run.stdout.splitlines():
        m = re.match(r"query (\d+) found (\d) outcome (-?\d+) carried (\d) subtree (\d+) collided (\d+) kept (\d+) "
                     r"depth (\d+) start (\d+) tree (\d+) rows (\d+) fnv ([0-9a-f]{16}) path(.*)", line)
        if m:
            got.append(dict(found=int(m[2]), outcome=int(m[3]), carried=int(m[4]),
                            rebase=[int(m[k]) for k in (5, 6, 7, 8)] if int(m[4]) else None, start=int(m[9]),
                            tree=int(m[10]), rows=int(m[11]), fnv=int(m[12], 16), ids=[int(v) for v in m[13].split()]))
    assert len(got) == 3
    return got


def _binding(carry):
    mode = abi.CLRRT_COLLISION_OBB
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 21, max_batch=BATCH,
                       max_obstacles=16)
    be = replan.PlannerBackend(pl, replan.default_make_params(mode), carry_tree=carry)
    rng = clrrt.Rng(SEED)
    out = []
    try:
        for st in STATES:
            pose = np.array(st)
            oc = be.begin_query(pose, replan.goal_in_car_frame(GOAL_W, pose),
                                replan.obstacles_in_car_frame(BOXES, 0.0, pose))
            rb = be.last_rebase
            start = pl.size()[0]
            pl.expand(rng, n_iters=BATCH * ROUNDS, mode=clrrt.CLRRT_MODE_BATCH, batch=BATCH)
            tree = pl.size()[0]
            ids, rows = be.end_query(pose)
            out.append(dict(found=int(len(ids) > 0), outcome=oc, carried=int(rb is not None),
                            rebase=None if rb is None else [rb["nodes_subtree"], rb["nodes_collided"], rb["nodes_kept"],
                                                            rb["depth"]],
                            start=start, tree=tree, rows=len(rows), fnv=_fnv1a(np.ascontiguousarray(rows).tobytes()),
                            ids=ids))
    finally:
        pl.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("carry", [True, False])
def test_native_plan_carry_matches_the_binding(carry):
    assert os.path.exists(EXE), "tests/native/plan_carry not built (make -C cl-rrt_amd/csrc)"
    got, want = _native(carry), _binding(carry)
    for q in range(3):
        assert got[q] == want[q], (q, got[q], want[q])
    assert got[0]["outcome"] == abi.REINIT_EMPTY and got[0]["found"]
    if carry:  # queries 1 and 2 start from the carried tree, which is more than the committed path
        for q in (1, 2):
            assert got[q]["carried"] and got[q]["start"] == got[q]["rebase"][2] > len(got[q - 1]["ids"])
    else:
        assert not any(g["carried"] for g in got) and got[1]["outcome"] == abi.REINIT_KEPT
