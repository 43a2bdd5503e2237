"""The oracle's batched checkObsDistance (orc_check_obs_n, the reference side of tests/test_collision_cull.py)
against its one-state form and a Python loop over getOBBdist.  CPU only."""
import math

import numpy as np

import collision_scenes as cs
from clrrt import abi, scenes
from oracle_binding import Oracle, obb_dist


def test_check_obs_n_matches_single_calls_and_obb_loop():
    obs = scenes.urban_scene(14, 6)
    o = Oracle(abi.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), obs)
    st = cs.uniform_states(obs, 300, seed=3)
    dist, first = o.check_obs_n(st)
    assert (dist == 0).sum() >= 30 and (dist != 0).sum() >= 30
    for i, x in enumerate(st):
        assert dist[i] == o.check_obs(x)
        veh = (x[0] + 1.424 * math.cos(x[2]), x[1] + 1.424 * math.sin(x[2]), 2.0, 4.848, x[2])
        want = -1
        for j, b in enumerate(obs):
            if obb_dist(veh, (b[0] + b[5] * x[6], b[1] + b[6] * x[6], b[3] / 2, b[4] / 2, b[2])) == 0:
                want = j
                break
        assert first[i] == want, (i, first[i], want)
        assert (dist[i] == 0) == (want >= 0)


def test_check_obs_n_stub_and_empty():
    st = cs.uniform_states(scenes.urban_scene(3), 8, seed=1)
    dist, first = Oracle(abi.default_params(), scenes.urban_scene(3)).check_obs_n(st)
    assert np.all(dist == 100) and np.all(first == -1)
    dist, first = Oracle(abi.default_params(collision_mode=abi.CLRRT_COLLISION_OBB)).check_obs_n(st)
    assert np.all(dist == 10000) and np.all(first == -1)
