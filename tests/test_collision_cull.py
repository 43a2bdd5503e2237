"""The rollout kernels' culled and reordered forms of checkObsDistance against the oracle's exhaustive one.

clrrt_selftest_collision runs the device functions of the step loops on explicit states: every obstacle
(obs_distance<true>), one lane over the static grid merged with the moving obstacles, the linear scan behind the
culls (grid withheld or absent), and the wave-cooperative check of the persistent kernel.  Per state the decision
(dist == 0) and the box-test count (first overlapping obstacle + 1, else the obstacle count) must equal the
oracle's; the exhaustive path's value equals it bit for bit.  The scenes reach the cell-list walk's odd tail, cell
lists longer than a 64-pair window, interleaved moving ids, absent and refused grids, states outside the grid and
on cell borders, first-contact states (the culls' 5 cm margin) and coordinates up to 2^22 m, where a float ulp
exceeds the margin.  The end-to-end tests run the real rollout kernels on the scenes with long cell lists.
"""
import numpy as np
import pytest

import clrrt
import collision_scenes as cs
from clrrt import abi
from oracle_binding import Oracle
from test_gpu_parity import _compare_trees

pytestmark = pytest.mark.gpu

PATHS = (("exhaustive", clrrt.Planner.COLL_EXHAUSTIVE), ("lane", clrrt.Planner.COLL_LANE),
         ("nogrid", clrrt.Planner.COLL_LANE_NOGRID), ("coop", clrrt.Planner.COLL_COOP))
_PL = []


def _planner():
    if not _PL:
        _PL.append(clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=1 << 10,
                                 max_rows=1 << 14, max_batch=64))
    return _PL[0]


def _setup(obs):
    pl = _planner()
    pl.set_obstacles(obs)
    g = pl.grid_info()
    # the cooperative check serves a rollout launch exactly when the query has a static grid (default options and
    # cost terms: no gap value needed, and the tables of a grid that was built leave room for the scratch)
    assert g["coop"] == (g["gw"] > 0)
    return pl, Oracle(abi.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), obs), g


def _check(pl, o, g, st, n_obs, label, active=None, paths=PATHS):
    """Every path on the states against the oracle; returns the oracle's (dist, first)."""
    odist, first = o.check_obs_n(st)
    hit = odist == 0
    act = np.ones(len(st), bool) if active is None else np.asarray(active, bool)
    assert np.array_equal(hit, first >= 0)
    want_tests = np.where(act, np.where(hit, first + 1, n_obs), 0).astype(np.uint32)
    res = {}
    for name, path in paths:
        if path == clrrt.Planner.COLL_COOP and not g["coop"]:
            with pytest.raises(clrrt.ClrrtError):
                pl.selftest_collision(path, st, active)
            continue
        dist, tests = pl.selftest_collision(path, st, active)
        res[name] = (dist, tests)
        bad = np.flatnonzero(act & ((dist == 0) != hit))
        print(f"{label} {name}: {len(st)} states, {int(hit[act].sum())} colliding, decision differs at {len(bad)}, "
              f"count differs at {int((tests != want_tests).sum())}")
        assert len(bad) == 0, (label, name, bad[:8], st[bad[:4], :3], odist[bad[:4]])
        assert np.all(dist[~act] == -1.0)
        if path == clrrt.Planner.COLL_EXHAUSTIVE:
            assert np.array_equal(dist[act].view(np.uint64), odist[act].view(np.uint64)), (label, name)
        else:
            assert np.all(dist[act & ~hit] == 10000.0)
        cb = np.flatnonzero(tests != want_tests)
        assert len(cb) == 0, (label, name, cb[:8], tests[cb[:8]], want_tests[cb[:8]])
    return odist, first, res


def _states(name, obs, o, g, n_uniform, contact=0, tmax=0.0):
    parts = [cs.uniform_states(obs, n_uniform, seed=11)]
    if g["gw"] > 0:
        parts.append(cs.grid_states(g, seed=12))
    if contact:
        parts.append(cs.first_contact_states(o, obs, contact, seed=13, tmax=tmax))
    parts.append(cs.nonfinite_block(parts[0]))
    st = np.concatenate(parts)
    assert len(st) <= 4096
    return st


def _run_scene(name, obs, n_uniform=1536, contact=0, tmax=0.0):
    pl, o, g = _setup(obs)
    st = _states(name, obs, o, g, n_uniform, contact, tmax)
    odist, first, res = _check(pl, o, g, st, len(obs), name)
    frac = float((odist == 0).mean())
    assert 0.10 <= frac <= 0.90, (name, frac)
    # the documented hook (clrrt_obstacle_distance) is the exhaustive path
    assert np.array_equal(pl.check_obs_distance(st).view(np.uint64), odist.view(np.uint64))
    # the non-finite lanes: NaN collides with the first obstacle, +inf with none (the reference's comparisons),
    # and their neighbours get what the same states got among finite lanes
    nb = len(st) - 64
    assert odist[nb + 5] == 0 and first[nb + 5] == 0 and odist[nb + 40] == 10000 and first[nb + 40] == -1
    keep = np.ones(64, bool)
    keep[[5, 40]] = False
    for pname, (dist, tests) in res.items():
        assert np.array_equal(dist[nb:][keep], dist[:64][keep]) and np.array_equal(tests[nb:][keep], tests[:64][keep])
    return pl, o, g, st, res


@pytest.mark.parametrize("name", ["single", "pair", "triple"])
def test_short_cell_lists(name):
    """Cell lists of 1, 2 and 3 obstacles: the two-at-a-time walk and its odd tail."""
    obs = cs.scene(name)
    pl, o, g, st, res = _run_scene(name, obs, contact=500 if name == "single" else 0)
    assert g["gw"] > 0 and g["nmov"] == 0
    assert int(np.diff(g["start"].astype(np.int64)).max()) == len(obs)


@pytest.mark.parametrize("name", ["stack", "stack_mov"])
def test_cell_lists_longer_than_a_window(name):
    """100 obstacles within a metre: every cell near them lists all the static ones, so a cooperative lane's
    pair range spans two 64-pair windows (the carried owner is live); stack_mov interleaves moving ids."""
    obs = cs.scene(name)
    pl, o, g, st, res = _run_scene(name, obs, contact=500, tmax=10.0 if name == "stack_mov" else 0.0)
    nstat = int((obs[:, 5:7] == 0).all(axis=1).sum())
    assert g["gw"] > 0 and g["nmov"] == len(obs) - nstat
    longest = int(np.diff(g["start"].astype(np.int64)).max())
    assert longest == nstat and longest > 64
    if name == "stack_mov":
        assert 0 < g["nmov"] and np.array_equal(g["mov"], np.arange(3, 100, 7))


def test_interleaved_moving_ids():
    """Every third obstacle moves: the merge of the cell list with the moving list decides the first overlap."""
    obs = cs.scene("interleaved")
    pl, o, g, st, res = _run_scene("interleaved", obs)
    assert g["gw"] > 0 and np.array_equal(g["mov"], np.arange(1, 60, 3))


def test_all_moving_has_no_grid():
    obs = cs.scene("all_moving")
    pl, o, g, st, res = _run_scene("all_moving", obs)
    assert g["gw"] == 0 and g["gh"] == 0 and g["nmov"] == 20 and not g["coop"] and "coop" not in res
    assert np.array_equal(res["lane"][0], res["nogrid"][0]) and np.array_equal(res["lane"][1], res["nogrid"][1])


@pytest.mark.parametrize("name", ["far_line", "far_L"])
def test_far_apart(name):
    """Obstacles 3000 m apart: a coarse grid, mostly empty cells, states around each obstacle and in the middle."""
    obs = cs.scene(name)
    pl, o, g, st, res = _run_scene(name, obs)
    assert g["gw"] > 0 and g["gw"] * g["gh"] <= 16384
    assert g["gw"] / float(g["inv"]) >= 3000.0
    if name == "far_L":
        assert g["gh"] / float(g["inv"]) >= 3000.0


@pytest.mark.parametrize("n,grid", [(1187, True), (1188, False), (1400, False)])
def test_capacity(n, grid):
    """The LDS budget of the grid: 120 KiB less 100 B per obstacle is 4180 B at 1187 obstacles and under the
    4 KiB floor from 1188, where the rollouts scan linearly behind the culls."""
    obs = cs.scene(f"capacity_{n}")
    pl, o, g = _setup(obs)
    assert (g["gw"] > 0) == grid and g["coop"] == grid
    u = cs.uniform_states(obs, 960, seed=11)
    st = np.concatenate([u, cs.nonfinite_block(u)])
    odist, first, res = _check(pl, o, g, st, n, f"capacity_{n}")
    assert len(st) == 1024 and 0.10 <= float((odist == 0).mean()) <= 0.90
    assert ("coop" in res) == grid


@pytest.mark.parametrize("off", cs.OFFSETS)
@pytest.mark.parametrize("name", ["single", "stack"])
def test_offset_coordinates(name, off):
    """The scene and its states moved by (off, -off).  Before obstacles beyond CULL_EXEMPT_BOUND (2^15 m) were exempt
    from culling, the lane path discarded colliding states from 2^18 m (1 of 962 colliding states of the single
    scene, 2 of 1169 of the stack), 62 and 76 at 2^20 m, 272 and 286 at 2^22 m: a float ulp there is a sizeable
    part of the culls' 5 cm margin, and the reference's float SAT still reports overlap.  4096 and 2^14 m lie
    below the bound (culled as ever), the others above it (exempt)."""
    obs = cs.shifted(cs.scene(name), off)
    pl, o, g, st, res = _run_scene(f"{name}+{off:g}", obs, contact=500)
    if off < cs.EXEMPT_BOUND:
        assert g["exempt"] == 0 and g["gw"] > 0 and g["nmov"] == 0
    else:
        assert g["exempt"] == len(obs) and g["gw"] == 0 and g["nmov"] == len(obs)


def test_exempt_obstacle_beside_a_grid():
    """Three obstacles near the origin and one at 2^20 m: the far one is exempt from culling and listed with the
    always-tested ids, the near ones keep their grid and the cooperative check."""
    obs = cs.scene("near_and_far")
    pl, o, g, st, res = _run_scene("near_and_far", obs, contact=500)
    assert g["exempt"] == 1 and g["gw"] > 0 and g["coop"] and np.array_equal(g["mov"], [3])
    assert g["gw"] / float(g["inv"]) < 100.0  # the grid spans the near obstacles only


def _lane_states(g, cells, rng):
    return np.stack([cs.state_in_cell(g, c, th=rng.uniform(-np.pi, np.pi), t=rng.uniform(0, 10)) for c in cells])


@pytest.mark.parametrize("name", ["urban60", "interleaved", "stack"])
def test_coop_wave_shapes(name):
    """Wave occupancies of the cooperative check: active-lane patterns, zero-length pair ranges first in the wave
    and between others, wave totals on and just past a window border, one long range among idle lanes."""
    obs = cs.scene(name)
    pl, o, g = _setup(obs)
    assert g["coop"]
    rng = np.random.RandomState(5)
    u = cs.uniform_states(obs, 64 * 6, seed=21)
    waves, acts = [], []

    def add(st, act):
        assert len(st) == 64 and len(act) == 64
        waves.append(st)
        acts.append(np.asarray(act, np.int32))

    lane = np.arange(64)
    add(u[0:64], np.ones(64))
    add(u[64:128], lane % 2 == 0)
    add(u[128:192], lane == 0)
    add(u[192:256], lane == 63)
    counts = cs.cell_counts(g)
    busy = max(counts)
    assert busy >= 1
    # zero-length ranges between non-empty ones: a busy cell, an active lane outside the grid (nmov candidates:
    # none without moving obstacles), an idle lane, in turn
    cells = np.where(lane % 3 == 0, counts[busy], -1)
    add(_lane_states(g, cells, rng), lane % 3 != 2)
    # zero-length ranges first in the wave
    first10 = u[256:320].copy()
    first10[:10] = _lane_states(g, [-1] * 10, rng)
    add(first10, np.where(lane < 5, 0, 1))
    # wave totals of exactly 64, 65 and 128 pairs: a window border on a range border, and just past one
    nmov = g["nmov"]
    per_lane = {c + nmov: cell for c, cell in counts.items() if c + nmov >= 1}
    if nmov >= 1:
        per_lane.setdefault(nmov, -1)
    for total in (64, 65, 128):
        lanes = cs.lanes_for_total(per_lane, total)
        assert lanes is not None, (name, total, sorted(per_lane))
        assert sum(lanes) == total
        # spread over the wave, idle lanes between them
        pos = np.linspace(0, 63, len(lanes)).astype(int) if len(lanes) > 1 else np.array([31])
        assert len(set(pos)) == len(lanes)
        cells = np.full(64, -1)
        cells[pos] = [per_lane[c] for c in lanes]
        act = np.zeros(64)
        act[pos] = 1
        add(_lane_states(g, cells, rng), act)
    if name == "stack":
        assert busy == 100
        add(_lane_states(g, [counts[100]] * 64, rng), lane == 17)   # one lane with 100 candidates, 63 idle
        add(_lane_states(g, [counts[100]] * 64, rng), np.ones(64))  # 64 lanes with 100 candidates each
    st, act = np.concatenate(waves), np.concatenate(acts)
    odist, first, res = _check(pl, o, g, st, len(obs), f"{name} waves", active=act,
                               paths=[p for p in PATHS if p[0] in ("lane", "coop")])
    assert "coop" in res
    assert np.array_equal(res["coop"][0], res["lane"][0]) and np.array_equal(res["coop"][1], res["lane"][1])
    a = act != 0
    assert (odist[a] == 0).sum() >= 0.1 * a.sum() and (odist[a] != 0).sum() >= 0.1 * a.sum()


# ---------------------------------------------------------------------------------------------- end to end
def _params():
    return abi.default_params(collision_mode=abi.CLRRT_COLLISION_OBB)


@pytest.mark.parametrize("name", ["stack", "stack_mov", "interleaved"])
def test_rollouts_through_long_cell_lists(name):
    """k_rollout on 200 jobs against Oracle.simulate, bit for bit (as test_gpu_parity._rollout_parity)."""
    obs = cs.scene(name)
    o = Oracle(_params(), obs)
    Oracle.srand(2)
    o.init_tree()
    o.expand(40)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=1 << 12,
                       max_rows=1 << 18, max_batch=256)
    pl.set_obstacles(obs)
    pl.tree_load(o.nodes_raw())
    jobs = []
    for s in clrrt.Rng(11).draw_samples(pl.params, 120):
        ids, _ = o.sort_nodes(s.x, s.y, s.explore)
        jobs += [(par, 0, s.x, s.y) for par in ids[:4]]
    jobs += [(par, 1, 0.0, 0.0) for par in range(o.size())]
    jobs = jobs[:200]
    assert len(jobs) == 200
    gpu = pl.simulate_batch(jobs, rows=True)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)  # noqa: E731
    outcomes = []
    for (par, gb, sx, sy), gr in zip(jobs, gpu):
        c = o.simulate(par, gb, sx, sy, rows=True)
        assert gr["outcome"] == c["outcome"] and gr["nrows"] == c["nrows"], (par, gb, gr["outcome"], c["outcome"])
        assert np.array_equal(bits(gr["final"]), bits(c["final"])) and np.array_equal(bits(gr["rows"]), bits(c["rows"]))
        assert gr["costE"] == c["costE"] and gr["costS"] == c["costS"]
        outcomes.append(c["outcome"])
    assert 3 in outcomes  # CLRRT_ROLL_COLLISION: some of the rollouts end in the obstacles
    pl.close()


def _batch_pair(name, sort_limit):
    """The oracle's BATCH tree of 4 rounds x 128 samples and the device's with roll_coop 1 and 0: the trees are
    equal; returns the two runs' work counters."""
    obs = cs.scene(name)
    q = _params()
    q.sort_limit = sort_limit
    o = Oracle(q, obs)
    Oracle.srand(6)
    o.init_tree()
    o.expand_batch(512, 128, stable=True)
    assert o.counters()["fail_collision"] > (100 if sort_limit > 1 else 20)
    work = []
    for coop in (1, 0):
        p = clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB)
        p.sort_limit = sort_limit
        pl = clrrt.Planner(p, max_nodes=1 << 14, max_rows=1 << 20, max_batch=128)
        pl.set_option("roll_coop", coop)
        pl.set_obstacles(obs)
        assert pl.grid_info(lists=False)["coop"] == bool(coop)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(6), n_iters=512, mode=clrrt.CLRRT_MODE_BATCH, batch=128)
        assert st["iterations"] == 512 and st["rounds"] == 4
        on, gn, bad = _compare_trees(o, pl, f"batch {name} sort_limit {sort_limit} coop {coop}")
        assert bad is None and len(on["parent"]) == len(gn["parent"])
        work.append(pl.work_counters())
        pl.close()
    print(f"batch {name} sort_limit {sort_limit}: work counters coop 1 {work[0]}, coop 0 {work[1]}")
    return work


@pytest.mark.parametrize("name", ["stack", "stack_mov", "interleaved"])
def test_batch_trees_through_long_cell_lists(name):
    """BATCH trees of 4 rounds x 128 samples with the cooperative check and without, against the oracle's."""
    _batch_pair(name, 10)


@pytest.mark.parametrize("name", ["stack", "stack_mov", "interleaved"])
def test_box_test_counter_independent_of_coop(name):
    """The box-test counter of whole expansions does not depend on which collision check ran.  Compared where the
    work itself is fixed: with one candidate per sample (sort_limit 1) every started rollout runs to its end.  With
    more, a later candidate is abandoned once an earlier one's success becomes visible to its lane (checked
    every 16 steps), so how many steps -- and box tests -- the abandoned ones ran depends on the schedule: on
    the stack scene two runs with the cooperative check counted 26190330 and 26174111 box tests (262013 steps in
    the second), one without 26106683 (261339 steps), for the same tree."""
    w1, w0 = _batch_pair(name, 1)
    assert w1["steps"] == w0["steps"] > 0
    assert w1["box_tests"] == w0["box_tests"] > 0
