"""Time-layered occupancy stacks (clrrt_set_occupancy_layers: one grid per time slice, a state tested against the layer
of its own time) -- GPU.

References: numpy (tests/occ_ref.py for the decision against one grid, tests/occ_layers_ref.py for the layer rule,
tests/clear_ref.py for the clearance), the engine's own single-grid mode, which tests/test_occ_gpu.py pins, and
tests/rebase_ref.py for the rebase bookkeeping.  Stacks, times and state sets come from tests/occ_layers_cases.py;
tests/test_occ_layers_host.py checks their input conditions on the CPU.  Time has no borderline band (the boundaries
are exact doubles); the only states skipped are occ_ref's borderline ones (|margin| <= 1e-9).
"""
import ctypes as C

import numpy as np
import pytest

import clear_ref
import clrrt
import occ_cases
import occ_layers_cases as lc
import occ_layers_ref as lr
import occ_ref
import rebase_ref
from clrrt import abi, scenes
from test_occ_gpu import _same_tree

pytestmark = pytest.mark.gpu

OCC, OBB, STUB = abi.CLRRT_COLLISION_OCC, abi.CLRRT_COLLISION_OBB, abi.CLRRT_COLLISION_STUB
T0, DT = lc.T0, lc.DT
G = 65536


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _set_stack(pl, grids, t0=T0, dt=DT):
    g = grids[0]
    pl.set_occupancy_layers(g.x0, g.y0, g.res, lc.cells3d(grids), t0, dt, g.inflate)


def _set_grid(pl, g):
    pl.set_occupancy(g.x0, g.y0, g.res, g.cells, g.inflate)


def _planner(params=None, **kw):
    cap = dict(max_nodes=1 << 12, max_rows=1 << 18, max_batch=256)
    cap.update(kw)
    return clrrt.Planner(params or clrrt.default_params(collision_mode=OCC), **cap)


@pytest.fixture
def guard():
    """Guard bands of 64 KiB around every device and pinned block of the planners the test appends; checked clean after
    they are closed."""
    clrrt.mem_check()
    clrrt.mem_guard(G)
    made = []
    try:
        yield made
        for pl in made:
            pl.close()
        rep = clrrt.mem_check()
        print(f"guard: {rep['blocks_checked']} blocks checked, {rep['violations']} violations")
        assert rep["violations"] == 0 and rep["blocks_checked"] > 0, rep
    finally:
        for pl in made:
            pl.close()
        clrrt.mem_guard(0)


_cases = {}


def _case(name):
    """(grids, states, margin per state against its layer, layer, margin against layer 0): numpy, computed once."""
    if name not in _cases:
        _, grids = lc.stacks()[name]
        st = lc.states(name)
        m, k = lr.margin_layers(st, grids, T0, DT)
        _cases[name] = (grids, st, m, k, occ_ref.margin(st, grids[0]))
    return _cases[name]


# ------------------------------------------------------------------------------------------------ 1. decision
@pytest.mark.parametrize("name", list(lc.stacks()))
def test_decision_per_layer_matches_numpy(name, guard):
    grids, st, m, k, m0 = _case(name)
    hit, skip = m <= 0.0, np.abs(m) <= occ_ref.BORDER
    keep = ~skip
    print(f"{name}: {len(grids)} layers, {hit.sum()} of {len(st)} states hit, {skip.sum()} borderline (skipped)")
    pl = _planner()
    guard.append(pl)
    _set_stack(pl, grids)
    li = pl.occupancy_layers_info()
    assert li["layers"] == len(grids) and (li["t0"], li["dt"]) == (T0, DT)
    want_occ = [int(np.count_nonzero(g.cells)) for g in grids]
    assert li["occupied"][:len(grids)] == want_occ and not any(li["occupied"][len(grids):])
    info = pl.occupancy_info()
    assert info["occupied"] == sum(want_occ) and info["map_bytes"] == li["map_bytes"]
    assert info["placement"] == li["placement"] == abi.OCC_LDS
    paths = (pl.COLL_EXHAUSTIVE, pl.COLL_LANE, pl.COLL_LANE_NOGRID, pl.COLL_COOP)
    # no obstacle list: 0 on a hit of the state's layer, else mode 1's value without obstacles (a rollout launch has
    # no cooperative check without a list: that path comes with the list below)
    want = np.where(hit, 0.0, 10000.0)
    got = pl.check_obs_distance(st)
    assert np.array_equal(got[keep], want[keep]), np.nonzero(keep & (got != want))[0][:8]
    for path in paths[:3]:
        d, t = pl.selftest_collision(path, st)
        assert np.array_equal(d[keep], want[keep]), (path, np.nonzero(keep & (d != want))[0][:8])
        assert not t.any()
    # obs_use_pred = 0: every state is decided by layer 0
    p0 = clrrt.default_params(collision_mode=OCC)
    p0.obs_use_pred = 0
    pl.set_params(p0)
    keep0 = np.abs(m0) > occ_ref.BORDER
    want0 = np.where(m0 <= 0.0, 0.0, 10000.0)
    assert ((m0 <= 0.0) != hit).sum() >= 64
    got = pl.check_obs_distance(st)
    assert np.array_equal(got[keep0], want0[keep0])
    for path in paths[:3]:
        d, t = pl.selftest_collision(path, st)
        assert np.array_equal(d[keep0], want0[keep0]), path
    # with the obstacle list: 0 on a grid hit (no box test made or counted), else mode 1's value, bit for bit
    pl.set_obstacles(scenes.urban_scene(200, 20))
    ref = {}
    pl.set_params(clrrt.default_params(collision_mode=OBB))
    assert pl.grid_info(lists=False)["coop"]
    ref["dist"] = pl.check_obs_distance(st)
    for path in paths:
        ref[path] = pl.selftest_collision(path, st)
    assert (ref["dist"] == 0).any() and (ref["dist"] != 0).any()
    pl.set_params(clrrt.default_params(collision_mode=OCC))
    got = pl.check_obs_distance(st)
    assert np.array_equal(_bits(got[keep]), _bits(np.where(hit, 0.0, ref["dist"])[keep]))
    for path in paths:
        d1, t1 = ref[path]
        d2, t2 = pl.selftest_collision(path, st)
        assert np.array_equal(_bits(d2[keep]), _bits(np.where(hit, 0.0, d1)[keep])), path
        assert np.array_equal(t2[keep], np.where(hit, 0, t1)[keep]), path


# ------------------------------------------------------------------------------------------------ 2. one layer
def _grow(pl, rounds=2, batch=256, seed=6):
    pl.tree_init(lc.gate_root())
    pl.reset_counters()
    st = pl.expand(clrrt.Rng(seed), n_iters=batch * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
    assert st["rounds"] == rounds, st
    return pl


def _gate_planner(setup, w2=0.0, clear_max=0.0, **kw):
    p = lc.gate_params(OCC)
    p.Wcost[2] = w2
    pl = _planner(p, max_nodes=1 << 14, max_rows=1 << 20, **kw)
    pl.set_option("defer_steps", 0)
    pl.set_occupancy_clearance(clear_max)
    setup(pl)
    return pl


def test_one_layer_is_todays_mode():
    g = occ_cases.wall_with_gap()
    _, st, _, _, _ = _case("k3_one_cell")
    a = _gate_planner(lambda pl: _set_grid(pl, g))
    b = _gate_planner(lambda pl: _set_stack(pl, [g]))
    try:
        ia, ib = a.occupancy_info(), b.occupancy_info()
        ia.pop("bake_ms"), ib.pop("bake_ms")
        assert ia == ib and ia["placement"] == abi.OCC_LDS
        la, lb = a.occupancy_layers_info(), b.occupancy_layers_info()
        assert la["layers"] == lb["layers"] == 1 and la["union_reach_bytes"] == lb["union_reach_bytes"] == 0
        assert la["occupied"] == lb["occupied"] and la["occupied"][0] == int(g.cells.sum())
        rs = lc.states("k3_one_cell")
        rs[:, 0] += 2.5  # around the wall
        assert np.array_equal(_bits(a.check_obs_distance(rs)), _bits(b.check_obs_distance(rs)))
        assert (a.check_obs_distance(rs) == 0).any()
        n = _same_tree(_grow(a), _grow(b), "set_occupancy | set_occupancy_layers with one layer")
        assert n > 30 and a.counters()["fail_collision"] > 0
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("clear_max", [0.0, 3.0], ids=["no_clearance", "clearance"])
def test_four_identical_layers_are_the_single_grid(clear_max):
    g = occ_cases.wall_with_gap()
    a = _gate_planner(lambda pl: _set_grid(pl, g), w2=2.0, clear_max=clear_max)
    b = _gate_planner(lambda pl: _set_stack(pl, [g] * 4), w2=2.0, clear_max=clear_max)
    try:
        assert b.occupancy_layers_info()["layers"] == 4
        assert b.occupancy_clearance_info()["baked"] == (clear_max > 0)
        n = _same_tree(_grow(a), _grow(b), "single grid | four identical layers")  # (costS included)
        nodes = a.nodes()
        assert n > 30 and len(set(nodes["costS"].tolist())) > 10
        rows = np.concatenate([a.rows(int(nodes["row_offset"][i]), int(nodes["nrows"][i])) for i in range(1, n)])
        assert len(np.unique(lr.layer_of(rows[:, 6], T0, DT, 4))) == 4  # the rows spread over every layer
    finally:
        a.close()
        b.close()


def test_set_occupancy_after_a_stack_leaves_one_layer_and_clearing_leaves_mode_1():
    grids, st, m, k, m0 = _case("k3_full_row")
    pl = _planner()
    try:
        pl.set_obstacles(scenes.urban_scene(200, 20))
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        ref = pl.check_obs_distance(st)
        pl.set_params(clrrt.default_params(collision_mode=OCC))
        _set_stack(pl, grids)
        assert pl.occupancy_layers_info()["layers"] == 3
        _set_grid(pl, grids[1])
        li = pl.occupancy_layers_info()
        assert li["layers"] == 1 and li["occupied"][0] == int(grids[1].cells.sum()) and not any(li["occupied"][1:])
        m1 = occ_ref.margin(st, grids[1])
        keep = np.abs(m1) > occ_ref.BORDER
        got = pl.check_obs_distance(st)
        assert np.array_equal(_bits(got[keep]), _bits(np.where(m1 <= 0, 0.0, ref)[keep]))
        _set_stack(pl, grids)
        pl.set_occupancy_layers(0.0, 0.0, 1.0, None, 0.0, 0.0)  # cleared: mode 2 is mode 1
        assert pl.occupancy_info()["w"] == 0 and pl.occupancy_info()["placement"] == abi.OCC_NONE
        assert pl.occupancy_layers_info()["layers"] == 0
        assert np.array_equal(_bits(pl.check_obs_distance(st)), _bits(ref))
        _set_stack(pl, grids)
        pl.set_occupancy(cells2d=None)
        assert pl.occupancy_layers_info()["layers"] == 0
        assert np.array_equal(_bits(pl.check_obs_distance(st)), _bits(ref))
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 3. placement
def _fill_stack(h, w, K, res, share, seed):
    return [occ_ref.Grid(2.0, -0.5 * h * res, res, occ_cases._random_fill(h, w, share, seed + k),
                         occ_ref.default_inflate(res)) for k in range(K)]


def _uniform_states(g, n, seed):
    """n states over the grid and a margin around it, x[6] from the times of the decision test."""
    rng = np.random.default_rng(seed)
    h, w = g.cells.shape
    st = occ_cases._state(rng.uniform(g.x0 - 4.0, g.x0 + w * g.res + 4.0, n),
                          rng.uniform(g.y0 - 4.0, g.y0 + h * g.res + 4.0, n), rng.uniform(-np.pi, np.pi, n))
    tt = lc.times()
    st[:, 6] = tt[np.arange(n) % len(tt)]
    return st


# K = 2 of 96 x 64: everything in LDS.  K = 8 of 512 x 512 (1 m cells, 1 % filled): the stack's bitmaps are 8 x 32 KiB,
# its union reach map 37 KiB -- the union alone goes to LDS.  K = 2 of 1100 x 1100 (1 m cells): the reach map of one
# layer is 1110 rows of 36 words, 156 KiB, above the 148 KiB rule -- the smallest stack whose union map does not fit
# (the 2048 x 512 x 16 stack of the caps test has a reach map of a few KiB per layer).
PLACEMENTS = [("lds", dict(h=64, w=96, K=2, res=0.25, share=0.05), abi.OCC_LDS),
              ("reach_lds", dict(h=512, w=512, K=8, res=1.0, share=0.01), abi.OCC_REACH_LDS),
              ("global", dict(h=1100, w=1100, K=2, res=1.0, share=0.01), abi.OCC_GLOBAL)]


@pytest.mark.parametrize("name,shape,placement", PLACEMENTS, ids=[p[0] for p in PLACEMENTS])
def test_placement_and_decisions_under_it(name, shape, placement):
    grids = _fill_stack(seed=40, **shape)
    st = _uniform_states(grids[0], 4096, 5)
    m, k = lr.margin_layers(st, grids, T0, DT)
    hit, keep = m <= 0.0, np.abs(m) > occ_ref.BORDER
    print(f"{name}: {hit.sum()} of {len(st)} hit, {(~keep).sum()} borderline, layers used {len(np.unique(k))}")
    assert 0.05 < hit.mean() < 0.95 and len(np.unique(k)) == shape["K"] and (~keep).mean() <= 0.005
    pl = _planner()
    try:
        _set_stack(pl, grids)
        li = pl.occupancy_layers_info()
        print(li)
        assert li["placement"] == placement and pl.occupancy_info()["placement"] == placement
        assert li["union_reach_bytes"] > 0 and li["map_bytes"] > 0
        if placement == abi.OCC_GLOBAL:
            assert li["union_reach_bytes"] > 148 * 1024
        elif placement == abi.OCC_REACH_LDS:
            assert li["map_bytes"] > 148 * 1024 > li["union_reach_bytes"]
        assert li["occupied"][:shape["K"]] == [int(g.cells.sum()) for g in grids]
        want = np.where(hit, 0.0, 10000.0)
        got = pl.check_obs_distance(st)
        assert np.array_equal(got[keep], want[keep]), np.nonzero(keep & (got != want))[0][:8]
        for path in (pl.COLL_EXHAUSTIVE, pl.COLL_LANE, pl.COLL_LANE_NOGRID):
            d, t = pl.selftest_collision(path, st)
            assert np.array_equal(d[keep], want[keep]), (path, np.nonzero(keep & (d != want))[0][:8])
        # a short obstacle list: the cooperative path runs with its scratch beside the maps, under the same placement
        pl.set_obstacles(scenes.urban_scene(20, 4))
        assert pl.occupancy_layers_info()["placement"] == placement
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        assert pl.grid_info(lists=False)["coop"]
        d1, t1 = pl.selftest_collision(pl.COLL_COOP, st)
        pl.set_params(clrrt.default_params(collision_mode=OCC))
        d2, t2 = pl.selftest_collision(pl.COLL_COOP, st)
        assert np.array_equal(_bits(d2[keep]), _bits(np.where(hit, 0.0, d1)[keep]))
        assert np.array_equal(t2[keep], np.where(hit, 0, t1)[keep])
        # the 220-obstacle list: its tables take LDS first, so the placement may step down; the decisions do not change
        pl.set_obstacles(scenes.urban_scene(200, 20))
        print(f"{name}: placement {placement} without an obstacle list, "
              f"{pl.occupancy_layers_info()['placement']} beside the tables of 220 obstacles")
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        d1, t1 = pl.selftest_collision(pl.COLL_COOP, st)
        pl.set_params(clrrt.default_params(collision_mode=OCC))
        d2, t2 = pl.selftest_collision(pl.COLL_COOP, st)
        assert np.array_equal(_bits(d2[keep]), _bits(np.where(hit, 0.0, d1)[keep]))
        assert np.array_equal(t2[keep], np.where(hit, 0, t1)[keep])
    finally:
        pl.close()


@pytest.mark.parametrize("name,shape,placement", PLACEMENTS[1:], ids=[p[0] for p in PLACEMENTS[1:]])
def test_rollouts_and_rounds_under_each_placement(name, shape, placement):
    """The rollout kernels themselves with the maps outside LDS (the gate tests run them with the maps in it): the one-lane-per-job kernel
    (simulate_batch) ends each rollout at the first row that hits the layer of its own time, and a round of the
    persistent kernel (expand) commits no row that does."""
    grids = _fill_stack(seed=40, **shape)
    jobs = occ_cases.rollout_jobs()
    pl = _planner(lc.gate_params(STUB), max_nodes=1 << 14, max_rows=1 << 20, max_batch=512)
    try:
        pl.tree_init(lc.gate_root())
        ref = pl.simulate_batch(jobs, rows=True)
        pl.set_params(lc.gate_params(OCC))
        _set_stack(pl, grids)
        assert pl.occupancy_layers_info()["placement"] == placement
        n_hit, n_free, n_skip = _check_gate_rollouts(pl, grids, ref)
        print(f"{name}: {n_hit} rollouts end at a cell, {n_free} free, {n_skip} borderline")
        assert n_hit >= 64 and n_free >= 64 and n_skip <= 2
        pl.set_option("defer_steps", 0)
        _grow(pl, rounds=1)
        nodes = pl.nodes()
        n = len(nodes["parent"])
        rows = np.concatenate([pl.rows(int(nodes["row_offset"][i]), int(nodes["nrows"][i]))[1:] for i in range(1, n)])
        m, k = lr.margin_layers(rows, grids, T0, DT)
        print(f"{name}: a round grew {n} nodes, {len(rows)} rows in layers {np.unique(k).tolist()}, smallest margin "
              f"{m.min():.3e}, {pl.counters()['fail_collision']} collisions")
        assert n > 10 and not (m <= -occ_ref.BORDER).any() and pl.counters()["fail_collision"] > 0
        assert len(np.unique(k)) >= (2 if shape["K"] > 2 else 1)  # (two layers of 0.5 s: a first round stays in layer 0)
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 4. the gate
def _check_gate_rollouts(pl, grids, ref):
    got = pl.simulate_batch(occ_cases.rollout_jobs(), rows=True)
    n_hit = n_free = n_skip = 0
    for j, (a, b) in enumerate(zip(ref, got)):
        k, border = lr.first_hit_row(a["rows"], grids, T0, DT)
        if border:
            n_skip += 1
            continue
        if k < 0:  # no reference hit: the rollout does not fail by collision -- it is the stub's rollout
            n_free += 1
            assert (b["outcome"], b["nrows"], b["ref_n"]) == (a["outcome"], a["nrows"], a["ref_n"]), j
            assert b["outcome"] != abi.ROLL_COLLISION
            assert _bits([b["costE"], b["costS"]]).tolist() == _bits([a["costE"], a["costS"]]).tolist(), j
            assert np.array_equal(_bits(b["rows"]), _bits(a["rows"])), j
        else:
            n_hit += 1
            assert b["outcome"] == abi.ROLL_COLLISION and b["nrows"] == k + 1, (j, k, b["outcome"], b["nrows"])
            assert np.array_equal(_bits(b["rows"][:k]), _bits(a["rows"][:k])), j
    return n_hit, n_free, n_skip


@pytest.mark.parametrize("gap", list(lc.GAPS))
@pytest.mark.parametrize("closing", [True, False], ids=["closing", "opening"])
def test_rollouts_through_a_gate(closing, gap, guard):
    grids = lc.gate(closing, gap)
    pl = _planner(lc.gate_params(STUB), max_batch=512)
    guard.append(pl)
    pl.tree_init(lc.gate_root())
    jobs = occ_cases.rollout_jobs()
    ref = pl.simulate_batch(jobs, rows=True)
    t_switch = T0 + lc.GATE_SWITCH * DT
    cross = [np.nonzero(a["rows"][:, 0] >= lc.WALL_X)[0] for a in ref]
    early = sum(1 for a, c in zip(ref, cross) if len(c) and a["rows"][c[0], 6] < t_switch)
    late = sum(1 for a, c in zip(ref, cross) if len(c) and a["rows"][c[0], 6] >= t_switch)
    assert early >= 16 and late >= 16, (early, late)
    pl.set_params(lc.gate_params(OCC))
    _set_stack(pl, grids)
    assert pl.occupancy_layers_info()["layers"] == lc.GATE_K
    n_hit, n_free, n_skip = _check_gate_rollouts(pl, grids, ref)
    print(f"{'closing' if closing else 'opening'} gate: {n_hit} rollouts end at the wall, {n_free} free, {n_skip} "
          f"borderline; {early} cross the wall plane before the switch, {late} after it")
    assert n_hit >= 16 and n_free >= 16 and n_skip <= 2
    # the layer decides: against the first layer alone, or the last alone, other rollouts would end at the wall (few of
    # the jobs steer through the gap beside the axis; through the one astride it, those still inside when it shuts)
    others = [sum(1 for a in ref if (occ_ref.first_hit_row(a["rows"], single)[0] >= 0) !=
                  (lr.first_hit_row(a["rows"], grids, T0, DT)[0] >= 0)) for single in (grids[0], grids[-1])]
    print(f"rollouts that would end otherwise against the first layer alone / the last alone: {others}")
    assert max(others) >= (8 if gap == "gap_m3_3" else 1)
    # the gap-value instantiation: Wcost[2] = 2 with the clearance on; collisions as before, costs from the layer
    p = lc.gate_params(OCC)
    p.Wcost[2] = 2.0
    pl.set_params(p)
    pl.set_occupancy_clearance(3.0)
    assert pl.occupancy_clearance_info()["baked"]
    assert pl.occupancy_layers_info()["field_bytes"] == 4 * grids[0].cells.size * lc.GATE_K
    ps = lc.gate_params(STUB)
    ps.Wcost[2] = 2.0
    pl.set_params(ps)
    ref2 = pl.simulate_batch(jobs, rows=True)
    pl.set_params(p)
    got = pl.simulate_batch(jobs, rows=True)
    n = 0
    for j, (a, b) in enumerate(zip(ref2, got)):
        k, border = lr.first_hit_row(a["rows"], grids, T0, DT)
        if border:
            continue
        if k >= 0:
            assert b["outcome"] == abi.ROLL_COLLISION and b["nrows"] == k + 1, j
            continue
        assert (b["outcome"], b["nrows"]) == (a["outcome"], a["nrows"]), j
        assert np.array_equal(_bits(b["rows"]), _bits(a["rows"])), j
        # costS: the term 2 exp(-4 min(Dobs, c)) per step with c the clearance on the row's own layer (Dobs: 10000
        # without obstacles), against the stub's 2 exp(-4 * 100); compared through the device's own clearance values
        c = pl.occupancy_clearance(b["rows"][1:])
        kk = lr.layer_of(b["rows"][1:, 6], T0, DT, lc.GATE_K)
        want, ok = np.empty(len(c)), np.ones(len(c), dtype=bool)
        for q in np.unique(kk):
            want[kk == q] = clear_ref.clearance(b["rows"][1:][kk == q], grids[q], 3.0)
            ok[kk == q] = ~clear_ref.borderline(b["rows"][1:][kk == q], grids[q])
        assert np.array_equal(_bits(c[ok]), _bits(want[ok])), j
        if len(np.unique(kk)) > 1 and (c < 3.0).any():
            n += 1
            assert b["costS"] > a["costS"]
    assert n >= 8


# ------------------------------------------------------------------------------------------------ 5. clearance
def test_clearance_per_layer():
    grids, st, m, k, _ = _case("k3_full_col")
    pl = _planner()
    try:
        pl.set_occupancy_clearance(4.0)
        _set_stack(pl, grids)
        ci = pl.occupancy_clearance_info()
        assert ci["baked"] and ci["field_bytes"] == 4 * 30 * 41 * 3
        fields = [clear_ref.field(g.cells) for g in grids]
        for q in range(3):
            assert np.array_equal(pl.occupancy_field(q), fields[q]), q
        assert np.array_equal(pl.occupancy_field(), fields[0])
        assert not np.array_equal(fields[0], fields[1]) and not np.array_equal(fields[1], fields[2])
        with pytest.raises(clrrt.ClrrtError):
            pl.occupancy_field(3)
        got = pl.occupancy_clearance(st)
        want = np.empty(len(st))
        for q in range(3):
            want[k == q] = clear_ref.clearance(st[k == q], grids[q], 4.0)
        skip = np.zeros(len(st), dtype=bool)
        for q in range(3):
            skip[k == q] = clear_ref.borderline(st[k == q], grids[q])
        print(f"clearance: {int(skip.sum())} states on a cell boundary within an ulp of the cosine")
        assert not skip.any()  # (no state of this set is near enough to a cell boundary for the cosine's ulp to matter)
        assert np.array_equal(_bits(got), _bits(want)), np.nonzero(_bits(got) != _bits(want))[0][:8]
        w0 = clear_ref.clearance(st, grids[0], 4.0)
        assert (_bits(w0) != _bits(want)).sum() >= 64  # the layer matters
        assert len(np.unique(want)) >= 8
        # obs_use_pred = 0: layer 0 for every state
        p0 = clrrt.default_params(collision_mode=OCC)
        p0.obs_use_pred = 0
        pl.set_params(p0)
        assert np.array_equal(_bits(pl.occupancy_clearance(st)), _bits(w0))
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 6. re-init, rebase
def _snapshot(pl):
    nodes = pl.nodes()
    n, nrows = pl.size()
    return nodes, pl.rows(0, nrows), bytes(pl.nodes_raw())


def _shifted_validity(pl, nodes, rows, t_shift):
    """From check_obs_distance (pinned to numpy by the decision test) on the rows with their time shifted (pose
    (0, 0, 0): positions stay): per node, whether one of its rows collides, and whether its last row does (all a
    rebase root keeps)."""
    dist = pl.check_obs_distance(rebase_ref.shift_rows(rows, (0.0, 0.0, 0.0), t_shift))
    off, nr = np.asarray(nodes["row_offset"], dtype=np.int64), np.asarray(nodes["nrows"], dtype=np.int64)
    any_row = np.array([bool((dist[o:o + r] == 0).any()) for o, r in zip(off, nr)])
    last_row = np.array([bool(dist[o + r - 1] == 0) for o, r in zip(off, nr)])
    return any_row, last_row


def test_rebase_revalidates_against_the_layer_of_the_shifted_time(guard):
    grids = lc.gate(True)
    pl = _gate_planner(lambda q: _set_stack(q, grids))
    guard.append(pl)
    _grow(pl)
    nodes, rows, raw = _snapshot(pl)
    n = len(nodes["parent"])
    assert n > 30
    # every row of the grown tree is clear of its own layer (borderline rows aside)
    m, _ = lr.margin_layers(rows, grids, T0, DT)
    assert not (m <= -occ_ref.BORDER).any()
    t_shift = -1.0  # the carried rows are a second later on the new clock: two layers on
    assert (lr.layer_of(rows[:, 6] - t_shift, T0, DT, lc.GATE_K) != lr.layer_of(rows[:, 6], T0, DT, lc.GATE_K)).any()
    # a root whose subtree loses nodes to the shift but which stays itself; and one whose own row is caught
    cnt = np.zeros(n, dtype=np.int64)
    for kk in range(n - 1, 0, -1):
        cnt[nodes["parent"][kk]] += cnt[kk] + 1
    any_row, last_row = _shifted_validity(pl, nodes, rows, t_shift)
    kept_case = coll_case = None
    for root in np.argsort(-cnt, kind="stable"):
        root = int(root)
        if root == 0:
            continue
        member, _, _, _ = rebase_ref.closure(nodes["parent"], root)
        invalid = any_row & member
        invalid[root] = last_row[root]
        if invalid[root] and coll_case is None:
            coll_case = root
        if not invalid[root] and kept_case is None and invalid.sum() >= 1 and member.sum() >= 4:
            mids = np.flatnonzero(member)
            off, nr = rebase_ref.node_rows(nodes, mids, root)
            kept_case = (root, member, invalid, mids, off, nr)
        if kept_case is not None and coll_case is not None:
            break
    assert kept_case is not None, "no subtree that the shift cuts without taking its root"
    assert coll_case is not None, "no node whose last row the shift moves into the closed gate"
    # ROOT_COLLIDES leaves the tree bit for bit
    c0 = pl.counters()
    info = pl.tree_rebase(coll_case, (0.0, 0.0, 0.0), t_shift)
    assert info["outcome"] == abi.REBASE_ROOT_COLLIDES, info
    n2, rows2, raw2 = _snapshot(pl)
    assert raw2 == raw and np.array_equal(_bits(rows2), _bits(rows)) and pl.counters() == c0
    # KEPT: the closure of the shifted validity
    root, member, invalid, mids, off, nr = kept_case
    _, kept, level, _ = rebase_ref.closure(nodes["parent"], root, invalid)
    ids, par = rebase_ref.renumber(kept, nodes["parent"], root)
    info = pl.tree_rebase(root, (0.0, 0.0, 0.0), t_shift)
    print(f"root {root}: {info}; {int((invalid & member).sum())} invalid of {int(member.sum())} members")
    assert info["outcome"] == abi.REBASE_KEPT, info
    assert info["nodes_subtree"] == int(member.sum()) and info["nodes_kept"] == len(ids) < int(member.sum())
    assert info["nodes_collided"] == int((invalid & member).sum())
    g = pl.nodes()
    assert np.array_equal(g["parent"], par)
    sel = np.searchsorted(mids, ids)
    assert np.array_equal(g["nrows"], nr[sel])
    want_rows = np.concatenate([rebase_ref.shift_rows(rows[off[i]:off[i] + nr[i]], (0.0, 0.0, 0.0), t_shift)
                                for i in sel])
    got_rows = pl.rows(0, pl.size()[1])
    assert np.array_equal(_bits(got_rows[:, 6]), _bits(want_rows[:, 6]))  # each row's own time after the shift
    assert np.array_equal(got_rows[:, :2], want_rows[:, :2])              # (pose (0, 0, 0): the positions stay)
    # and the rows that stayed are clear of the layer of their new time
    m2, _ = lr.margin_layers(got_rows, grids, T0, DT)
    assert not (m2 <= -occ_ref.BORDER).any()


def test_reinit_checks_each_path_row_against_its_layer():
    """A committed path grown in an empty world crosses the plane x = 16 during some time slices.  A stack with a whole
    wall in exactly those layers erases the path, as the single grid with the wall does; a stack with the wall in every
    OTHER layer keeps it, as the empty single grid does."""
    def planner():
        pl = clrrt.Planner(clrrt.default_params(collision_mode=OCC), max_nodes=1 << 16, max_rows=1 << 22, max_batch=256)
        pl.tree_init()
        pl.expand(clrrt.Rng(4), n_iters=256 * 6, mode=clrrt.CLRRT_MODE_BATCH, batch=256)  # an empty world
        ids, _, ngoal = pl.extract_best_path()
        assert ngoal > 0 and len(ids) >= 3
        pl.path_commit(ids)
        return pl

    a, b = planner(), planner()
    try:
        hdr, prow = a.path_download()
        wall = lc.gate(False)[0]  # the wall without a gap
        empty = wall._replace(cells=np.zeros_like(wall.cells))
        mw = occ_ref.margin(prow, wall)
        assert (mw <= 0).any() and (np.abs(mw) > occ_ref.BORDER).all()
        K = 16
        at = np.unique(lr.layer_of(prow[mw <= 0, 6], T0, DT, K))
        print(f"the path's rows inside the wall lie in layers {at.tolist()} of {K}")
        assert 0 < len(at) < K and at.max() < K - 1
        car = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        _set_stack(a, [wall if q in at else empty for q in range(K)])
        _set_grid(b, wall)
        oa, ob = a.tree_init_from_path(car), b.tree_init_from_path(car)
        assert oa == ob == abi.REINIT_COLLISION
        assert bytes(a.nodes_raw()) == bytes(b.nodes_raw()) and a.size() == b.size() == (1, 1)
        _set_stack(a, [empty if q in at else wall for q in range(K)])
        _set_grid(b, empty)
        a.path_load(hdr, prow)
        b.path_load(hdr, prow)
        oa, ob = a.tree_init_from_path(car), b.tree_init_from_path(car)
        assert oa == ob == abi.REINIT_KEPT
        assert bytes(a.nodes_raw()) == bytes(b.nodes_raw()) and a.size() == b.size() and a.size()[0] > 1
        assert np.array_equal(_bits(a.rows(0, a.size()[1])), _bits(b.rows(0, b.size()[1])))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 7. expansion
@pytest.mark.parametrize("variant", [dict(exact=64), dict(defer_steps=128)], ids=["exact_64", "batch_T128"])
def test_expansion_under_the_gate(variant):
    grids = lc.gate(True)

    def run():
        pl = _gate_planner(lambda q: _set_stack(q, grids))
        pl.set_option("defer_steps", variant.get("defer_steps", 0))
        pl.tree_init(lc.gate_root())
        if "exact" in variant:
            st = pl.expand(clrrt.Rng(6), n_iters=variant["exact"], mode=clrrt.CLRRT_MODE_EXACT, batch=256)
            assert st["iterations"] == variant["exact"]
        else:
            pl.expand(clrrt.Rng(6), n_iters=512, mode=clrrt.CLRRT_MODE_BATCH, batch=256)
        return pl

    a, b = run(), run()
    try:
        n = _same_tree(a, b, "two runs under the closing gate")
        assert n > 10
        nodes = a.nodes()
        rows = np.concatenate([a.rows(int(nodes["row_offset"][i]), int(nodes["nrows"][i]))[1:] for i in range(1, n)])
        m, k = lr.margin_layers(rows, grids, T0, DT)
        print(f"{n} nodes, {len(rows)} rows in layers {np.unique(k).tolist()}, smallest margin {m.min():.3e}, "
              f"{a.counters()['fail_collision']} collisions")
        assert not (m <= -occ_ref.BORDER).any()
        assert len(np.unique(k)) >= 4 and a.counters()["fail_collision"] > 0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 8. caps, errors
def test_stack_at_the_caps_counts_its_cells():
    K, h, w = 16, 512, 2048
    cells = (np.random.default_rng(9).random((K, h, w)) < 0.02).astype(np.uint8)
    pl = _planner()
    try:
        pl.set_occupancy_layers(0.0, -25.6, 0.1, cells, T0, DT, 0.0)
        li = pl.occupancy_layers_info()
        print({k: v for k, v in li.items() if k != "occupied"})
        assert li["layers"] == K and li["occupied"] == cells.reshape(K, -1).sum(axis=1).tolist()
        assert pl.occupancy_info()["occupied"] == int(cells.sum())
        assert li["placement"] in (abi.OCC_REACH_LDS, abi.OCC_GLOBAL)
        # a few states per layer, against numpy
        g = [occ_ref.Grid(0.0, -25.6, 0.1, cells[q], 0.0) for q in range(K)]
        st = _uniform_states(g[0], 512, 3)
        m, _ = lr.margin_layers(st, g, T0, DT)
        keep = np.abs(m) > occ_ref.BORDER
        assert np.array_equal(pl.check_obs_distance(st)[keep], np.where(m <= 0, 0.0, 10000.0)[keep])
    finally:
        pl.close()


def test_set_occupancy_layers_validates_its_input():
    grids, st, m, k, _ = _case("k3_full_row")
    pl = _planner()
    try:
        _set_stack(pl, grids)
        before = (pl.occupancy_info(), pl.occupancy_layers_info(), pl.check_obs_distance(st))
        cells = np.zeros(2 * 64, np.uint8)
        ptr = C.c_void_p(cells.ctypes.data)

        def rc(layers=2, t0=0.25, dt=0.5, w=8, h=8, res=0.5, p=ptr):
            o = abi.Occupancy(0.0, 0.0, res, 0.0, w, h)
            r = pl.L.clrrt_set_occupancy_layers(pl.h, C.byref(o), layers, t0, dt, p)
            return r, pl.L.clrrt_last_error(pl.h).decode()

        for kw, word in ((dict(layers=0), "layers"), (dict(layers=17), "layers"), (dict(layers=-1), "layers"),
                         (dict(w=2048, h=2048, layers=5), "layers"), (dict(w=1024, h=1025, layers=16), "layers"),
                         (dict(dt=0.0), "dt"), (dict(dt=-0.5), "dt"), (dict(dt=np.nan), "dt"), (dict(dt=np.inf), "dt"),
                         (dict(t0=np.inf), "t0"), (dict(t0=np.nan), "t0"), (dict(p=None), "cells"),
                         (dict(w=2049), "w"), (dict(h=0), "h"), (dict(res=0.0), "res")):
            r, msg = rc(**kw)
            assert r == -1 and "set_occupancy_layers:" in msg, (kw, r, msg)
            assert word in msg.split("set_occupancy_layers:")[1].replace("*", " ").split()[0:5], (kw, msg)
            # the context is unchanged
            assert pl.occupancy_info() == before[0] and pl.occupancy_layers_info() == before[1], kw
        assert np.array_equal(_bits(pl.check_obs_distance(st)), _bits(before[2]))
        assert rc()[0] == 0 and pl.occupancy_layers_info()["layers"] == 2
        assert rc(w=0)[0] == 0 and pl.occupancy_layers_info()["layers"] == 0  # w == 0 clears
    finally:
        pl.close()
