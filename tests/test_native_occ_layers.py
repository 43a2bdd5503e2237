"""planMotion with a stack of occupancy time layers through the C++ adapter (OccupancyGrid::layers -> MotionPlanner::
updateOccupancy -> clrrt_set_occupancy_layers, include/clrrt_adapter.hpp) with no Python in the loop
(tests/native/occ_layers_plan.cpp): a stack of four identical layers returns the single grid's MPC message byte for
byte, and under the gate that closes the query completes with a committed path none of whose rows collides with the
layer of its own time."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "occ_layers_plan")
SEED, BATCH, ROUNDS = 11, 256, 6


def test_occ_layers_plan_program_compiles():
    """CPU: the adapter with the layered grid and the program compile (host C++ only)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "occ_layers_plan.cpp")], check=True)


@pytest.mark.gpu
def test_native_planmotion_with_a_stack():
    assert os.path.exists(EXE), "tests/native/occ_layers_plan not built (make -C cl-rrt_amd/csrc)"
    run = subprocess.run([EXE, str(SEED), str(BATCH), str(ROUNDS)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    got = {}
    for line in run.stdout.splitlines():
        m = re.match(r"query (\w+) found (\d) layers (\d+) tree (\d+) collisions (\d+) msg (\d+) rows (\d+) colliding (\d+) "
                     r"tmax ([0-9.]+) same (\d)", line)
        if m:
            got[m[1]] = dict(found=int(m[2]), layers=int(m[3]), tree=int(m[4]), collisions=int(m[5]), msg=int(m[6]),
                             rows=int(m[7]), colliding=int(m[8]), tmax=float(m[9]), same=int(m[10]))
    assert set(got) == {"single", "same4", "gate"}
    s, f, g = got["single"], got["same4"], got["gate"]
    assert (s["layers"], f["layers"], g["layers"]) == (1, 4, 8)
    # four identical layers: the single grid's query, message included
    assert s["found"] and s["msg"] >= 3 and s["collisions"] > 0
    assert f["same"] == 1 and {k: v for k, v in f.items() if k != "layers"} == {k: v for k, v in s.items() if k != "layers"}
    assert s["tmax"] > 0.25 + 3 * 0.5  # the path's rows reach past the fourth layer: every layer was read
    # the gate: the query completes, and no row of what it committed collides
    assert g["found"] and g["msg"] >= 3 and g["rows"] > 0
    assert g["colliding"] == 0 and g["collisions"] > 0
    assert g["tmax"] > 0.25 + 4 * 0.5  # the path goes on past the time at which the gap shuts
    assert g["collisions"] != s["collisions"]  # the gap that closes takes rollouts the open one lets through
