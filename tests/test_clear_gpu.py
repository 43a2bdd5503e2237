"""Occupancy clearance (clrrt_set_occupancy_clearance: the grid's distance field and the clearance in the obstacle
cost term) -- GPU.

The references are numpy (tests/clear_ref.py: the field as a brute force over the occupied cells, the clearance as
the header states it) and the engine with clearance off.  The grids and state sets are those of tests/occ_cases.py
plus clear_ref.extra_states; tests/test_clear_host.py checks their input conditions on the CPU.  A state with a circle
centre within 1e-9 cell of a cell boundary that an ulp of the cosine or sine moves into the neighbouring cell
(clear_ref.borderline) is the only kind of state a test here skips: the device's cosine may differ from numpy's by an
ulp.  clrrt_simulate runs the k_rollout template that clrrt_rollout_batch (test 4) and the speculative rounds (test 5)
instantiate, with the same step function.
"""
import math

import numpy as np
import pytest

import clrrt
import clear_ref
import occ_cases
import occ_ref
from clrrt import abi, scenes
from test_clear_host import sets
from test_gpu_parity import _nn_strategy

pytestmark = pytest.mark.gpu

OCC, OBB = abi.CLRRT_COLLISION_OCC, abi.CLRRT_COLLISION_OBB
ESTATE = -4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _set_grid(pl, g):
    pl.set_occupancy(g.x0, g.y0, g.res, g.cells, g.inflate)


def _planner(params=None, **kw):
    kw = dict(dict(max_nodes=1 << 10, max_rows=1 << 14, max_batch=64), **kw)
    return clrrt.Planner(params if params is not None else clrrt.default_params(collision_mode=OCC), **kw)


def _params(w2, mode=OCC):
    p = clrrt.default_params(collision_mode=mode)
    p.Wcost[2] = w2
    return p


# ------------------------------------------------------------------------------------------------ 1. field
def _field_grids():
    out = {k: v[0] for k, v in occ_cases.grids().items() if k != "random_1024"}
    corner = np.zeros((70, 33), np.uint8)  # one word and one bit per row; the occupied cell in the last row's last bit
    corner[69, 32] = 1
    out["corner_33x70"] = occ_ref.Grid(0.0, 0.0, 0.5, corner, 0.0)
    wide = (np.random.default_rng(5).random((3, 2048)) < 0.01).astype(np.uint8)  # 64 words per row, three rows
    wide[1, 2047] = 1
    wide[:, 700:1500] = 0  # a run of empty words: the nearest occupied word is many words away
    out["wide_2048x3"] = occ_ref.Grid(0.0, 0.0, 0.1, wide, 0.0)
    return out


@pytest.mark.parametrize("name", list(_field_grids()))
def test_field_matches_brute_force(name):
    g = _field_grids()[name]
    want = clear_ref.field(g.cells)
    pl = _planner()
    try:
        _set_grid(pl, g)
        assert pl.occupancy_clearance_info() == dict(clear_max=0.0, on=0, baked=0, field_bytes=0, bake_ms=0.0)
        assert pl.L.clrrt_occupancy_field(pl.h, want.ctypes.data) == ESTATE
        pl.set_occupancy_clearance(3.0)
        info = pl.occupancy_clearance_info()
        print(f"{name}: field bake {info['bake_ms']:.4f} ms, {int(np.count_nonzero(g.cells))} occupied cells")
        assert (info["clear_max"], info["on"], info["baked"], info["field_bytes"]) == (3.0, 1, 1, 4 * g.cells.size)
        got = pl.occupancy_field()
        assert got.dtype == np.uint32 and got.shape == g.cells.shape
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        if not g.cells.any():
            assert (got == 0xFFFFFFFF).all()
    finally:
        pl.close()


def test_field_follows_the_grid_and_is_freed_when_off():
    grids = _field_grids()
    a, b = grids["random_96x64"], grids["full_col"]
    pl = _planner()
    try:
        pl.set_occupancy_clearance(2.0)  # before any grid: on, nothing to bake
        info = pl.occupancy_clearance_info()
        assert (info["on"], info["baked"], info["field_bytes"]) == (1, 0, 0)
        assert pl.L.clrrt_occupancy_field(pl.h, None) == -1
        _set_grid(pl, a)
        assert np.array_equal(pl.occupancy_field(), clear_ref.field(a.cells))
        _set_grid(pl, b)  # replacing the grid re-bakes the field
        assert pl.occupancy_clearance_info()["field_bytes"] == 4 * b.cells.size
        assert np.array_equal(pl.occupancy_field(), clear_ref.field(b.cells))
        pl.set_occupancy(cells2d=None)  # no grid: no field
        assert pl.occupancy_clearance_info()["baked"] == 0
        _set_grid(pl, a)
        assert np.array_equal(pl.occupancy_field(), clear_ref.field(a.cells))
        pl.set_occupancy_clearance(0.0)  # off: freed
        info = pl.occupancy_clearance_info()
        assert (info["clear_max"], info["on"], info["baked"], info["field_bytes"]) == (0.0, 0, 0, 0)
        out = np.zeros(a.cells.shape, np.uint32)
        assert pl.L.clrrt_occupancy_field(pl.h, out.ctypes.data) == ESTATE
        assert "no field" in pl.L.clrrt_last_error(pl.h).decode()
        _set_grid(pl, b)  # and a later grid bakes none
        assert pl.occupancy_clearance_info()["baked"] == 0
        for bad in (-1.0, math.nan, math.inf):
            assert pl.L.clrrt_set_occupancy_clearance(pl.h, bad) == -1
            assert "clear_max" in pl.L.clrrt_last_error(pl.h).decode()
        assert pl.occupancy_clearance_info()["on"] == 0
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 2. clearance
@pytest.mark.parametrize("name", list(occ_cases.grids()))
def test_clearance_matches_numpy(name):
    g0, ss = sets(name)
    st = np.concatenate([ss["states"], ss["extra"]])
    skip = np.concatenate([clear_ref.borderline(s, g0) for s in ss.values()])  # (inflate does not enter)
    print(f"{name}: {skip.sum()} of {len(st)} states borderline (skipped)")
    assert skip[:4096].mean() <= 0.01 and skip[4096:].mean() <= 0.01
    keep = ~skip
    pl = _planner()
    try:
        for inflate in (0.0, occ_ref.default_inflate(g0.res), 0.3):
            g = g0._replace(inflate=inflate)
            _set_grid(pl, g)
            for clear_max in (3.0, 0.5):
                pl.set_occupancy_clearance(clear_max)
                got = pl.occupancy_clearance(st)
                want = clear_ref.clearance(st, g, clear_max)
                bad = np.nonzero(keep & (_bits(got) != _bits(want)))[0]
                assert len(bad) == 0, (inflate, clear_max, bad[:8], got[bad[:8]], want[bad[:8]])
                assert (got[~np.isfinite(st[:, :3]).all(axis=1)] == clear_max).all()
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 3. nothing else
@pytest.mark.parametrize("name", ["one_cell", "full_col", "random_96x64"])
def test_collision_decision_and_hook_are_unchanged(name):
    g, ss = sets(name)
    st = ss["states"]
    # Wcost[2] = 2: the gap-value rollouts, which take no cooperative check; the default 0: all four paths
    for w2 in (2.0, 0.0):
        pl = _planner(_params(w2))
        try:
            _set_grid(pl, g)
            pl.set_obstacles(scenes.urban_scene(200, 20))
            paths = (pl.COLL_EXHAUSTIVE, pl.COLL_LANE, pl.COLL_LANE_NOGRID) + ((pl.COLL_COOP,) if w2 == 0.0 else ())

            def snapshot():
                return [pl.check_obs_distance(st)] + [pl.selftest_collision(p, st) for p in paths]

            off = snapshot()
            pl.set_occupancy_clearance(3.0)
            assert pl.occupancy_clearance_info()["baked"] == 1
            on = snapshot()
            assert (off[0] == 0).any() and (off[0] != 0).any()
            assert np.array_equal(_bits(on[0]), _bits(off[0]))
            for (d1, t1), (d2, t2) in zip(off[1:], on[1:]):
                assert np.array_equal(_bits(d2), _bits(d1)) and np.array_equal(t2, t1)
        finally:
            pl.close()


# ------------------------------------------------------------------------------------------------ 4. cost
def test_rollout_cost_is_the_sum_of_the_clearance_terms():
    """Every outcome but ROLL_COLLISION has all of its logged rows after the start row costed: roll_step_post returns
    a collision before the cost lines and every other outcome after them.  So the rollouts compared are those that
    succeed (end, goal) and, being costed in full as well, those that end at the acceleration or iteration limit."""
    W2, W3, CLEAR_MAX = 2.0, 1.5, 3.0
    g = occ_cases.wall_with_gap()
    jobs = occ_cases.rollout_jobs()
    p = clrrt.default_params(collision_mode=OCC)
    for k, v in enumerate((0.0, 0.0, W2, W3, 1.0)):
        p.Wcost[k] = v
    assert p.bend == 0
    pl = _planner(p, max_batch=512)
    try:
        pl.tree_init()
        _set_grid(pl, g)
        off = pl.simulate_batch(jobs, rows=True)
        pl.set_occupancy_clearance(CLEAR_MAX)
        on = pl.simulate_batch(jobs, rows=True)
        pl.set_occupancy_clearance(0.0)
        off2 = pl.simulate_batch(jobs, rows=True)
        n_cmp = n_skip = n_coll = n_moved = 0
        args = []
        for j, (a, b, a2) in enumerate(zip(off, on, off2)):
            # outcomes, nrows, rows and costE: the clearance-off run's, by bits
            assert (b["outcome"], b["nrows"], b["ref_n"]) == (a["outcome"], a["nrows"], a["ref_n"]), j
            assert np.array_equal(_bits(b["rows"]), _bits(a["rows"])), j
            assert np.array_equal(_bits(b["final"]), _bits(a["final"])), j
            assert _bits([b["costE"]]).tolist() == _bits([a["costE"]]).tolist(), j
            assert _bits([a2["costS"]]).tolist() == _bits([a["costS"]]).tolist(), j
            if a["outcome"] == abi.ROLL_COLLISION:
                n_coll += 1
                continue
            rows = a["rows"][1:]
            # clearance off: no obstacle list, so every step's term is W2 exp(-W3 10000) = +0
            assert a["costS"] == 0.0, j
            if clear_ref.borderline(rows, g).any():
                n_skip += 1
                continue
            c = clear_ref.clearance(rows, g, CLEAR_MAX)
            want = 0.0
            for ci in c:
                x = -W3 * min(10000.0, float(ci))
                args.append(x)
                want += 0.0 + W2 * math.exp(x)
            assert _bits([b["costS"]]).tolist() == _bits([want]).tolist(), (j, b["costS"], want)
            n_cmp += 1
            n_moved += b["costS"] > 0.0
        # the engine's exp is the C library's on the arguments used
        args = np.unique(np.array(args))
        assert np.array_equal(_bits(pl.selftest_math(6, args)), _bits([math.exp(x) for x in args]))
        print(f"rollouts: {n_cmp} compared, {n_coll} collide, {n_skip} with a borderline row")
        assert n_cmp >= 100 and n_coll >= 100 and n_moved >= 100
        assert n_skip <= 0.01 * (n_cmp + n_skip)
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 5. trees
def _cfg3_grid(x0=15.0):
    """The cfg3 boxes rasterised; the window begins 15 m ahead of the root, so the first nodes' circles lie outside
    the grid and read clear_max."""
    obs = scenes.urban_scene(200, 20)
    y0, res, h = -26.0, 0.2, 260
    w = int(round((66.0 - x0) / res))
    cells = scenes.rasterize(obs, x0, y0, res, w, h)
    return obs[200:], occ_ref.Grid(x0, y0, res, cells, occ_ref.default_inflate(res))


# clear_max at mode 1's "no obstacle" distance: a row whose clearance is clear_max then takes min(Dobs, c) = Dobs
TREE_CLEAR_MAX = 10000.0
TREES = [dict(nn="brute", opts=dict(defer_steps=0)), dict(nn="walk", opts=dict(defer_steps=32, nn_lag=2))]


def _grow(variant, movers, grid, clear_max, batch=256, rounds=4, seed=6):
    pl = _planner(_params(2.0), max_nodes=1 << 16, max_rows=1 << 21, max_batch=batch)
    for k, v in variant["opts"].items():
        pl.set_option(k, v)
    _nn_strategy(pl, variant["nn"])
    pl.set_obstacles(movers)
    _set_grid(pl, grid)
    pl.set_occupancy_clearance(clear_max)
    pl.tree_init()
    rng = clrrt.Rng(seed)
    st = pl.expand(rng, n_iters=batch * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
    assert st["rounds"] == rounds, st
    return pl, bytes(rng.state)


@pytest.mark.parametrize("variant", TREES, ids=["batch_T0_brute", "batch_T32_walk_lag2"])
def test_tree_is_the_clearance_off_tree_but_for_costS(variant):
    movers, g = _cfg3_grid()
    assert np.count_nonzero(g.cells) > 3000
    a, rng_a = _grow(variant, movers, g, 0.0)
    b, rng_b = _grow(variant, movers, g, TREE_CLEAR_MAX)
    try:
        an, bn = a.nodes(), b.nodes()
        n = len(an["parent"])
        assert n == len(bn["parent"]) and n > 50
        assert rng_a == rng_b and a.counters() == b.counters()
        for k in ("parent", "goal", "nrows", "owner", "row_offset"):
            assert np.array_equal(an[k], bn[k]), k
        assert np.array_equal(an["costE"].view(np.uint32), bn["costE"].view(np.uint32))
        for k in ("state", "ref_front", "ref_back", "ref_vback", "ang_par"):
            assert np.array_equal(_bits(an[k]), _bits(bn[k])), k
        nr = a.size()[1]
        assert a.size() == b.size()
        rows = a.rows(0, nr)
        assert np.array_equal(_bits(rows), _bits(b.rows(0, nr)))
        assert (bn["costS"] >= an["costS"]).all()
        assert (bn["costS"] > an["costS"]).any()
        # a node all of whose rows, and its ancestors', read clear_max costs what it costs with clearance off
        c = clear_ref.clearance(rows, g, TREE_CLEAR_MAX)
        free = np.zeros(n, bool)
        free[0] = True
        for i in range(1, n):  # (a parent precedes its children)
            r0, k = int(an["row_offset"][i]), int(an["nrows"][i])
            free[i] = free[int(an["parent"][i])] and bool((c[r0 + 1:r0 + k] == TREE_CLEAR_MAX).all())
        print(f"{n} nodes, {free.sum()} with every row at clear_max, {(bn['costS'] > an['costS']).sum()} cost more")
        assert free[1:].sum() >= 5 and not free.all()
        assert np.array_equal(an["costS"][free].view(np.uint32), bn["costS"][free].view(np.uint32))
    finally:
        a.close()
        b.close()


def test_reinit_cost_takes_the_clearance():
    pl = _planner(_params(2.0), max_nodes=1 << 16, max_rows=1 << 22, max_batch=256)
    try:
        pl.tree_init()
        pl.expand(clrrt.Rng(4), n_iters=256 * 6, mode=clrrt.CLRRT_MODE_BATCH, batch=256)  # no grid yet
        ids, _, ngoal = pl.extract_best_path()
        assert ngoal > 0 and len(ids) >= 3
        pl.path_commit(ids)
        hdr, prow = pl.path_download()
        third = hdr[2]
        seg = prow[third.row_offset:third.row_offset + third.nrows]
        # a window of 40 x 40 cells of 0.25 m with one occupied cell 2.5 m to the side of a row of the path's third
        # node: near the path (the circles come within about 1.2 m) and clear of the box by numpy's margin; rows more
        # than 5 m up or down the path lie outside the window and read clear_max
        res, nw = 0.25, 40
        for r in seg[len(seg) // 2:]:
            cs, sn = np.cos(r[2]), np.sin(r[2])
            cx, cy = r[0] + occ_ref.OFF * cs + 2.5 * sn, r[1] + occ_ref.OFF * sn - 2.5 * cs
            x0, y0 = cx - (nw // 2 + 0.5) * res, cy - (nw // 2 + 0.5) * res
            cells = np.zeros((nw, nw), np.uint8)
            cells[nw // 2, nw // 2] = 1
            g = occ_ref.Grid(x0, y0, res, cells, 0.0)
            c = clear_ref.clearance(prow, g, TREE_CLEAR_MAX)
            if (occ_ref.margin(prow, g) > 0.011).all() and c.min() < 1.5 and not clear_ref.borderline(prow, g).any():
                break
        else:
            raise AssertionError("no row with the cell clear of the box and near the circles")
        _set_grid(pl, g)
        car = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        assert pl.tree_init_from_path(car) == abi.REINIT_KEPT
        off = pl.nodes()
        off_raw = bytes(pl.nodes_raw())
        pl.path_load(hdr, prow)
        pl.set_occupancy_clearance(TREE_CLEAR_MAX)
        assert pl.tree_init_from_path(car) == abi.REINIT_KEPT
        on = pl.nodes()
        n = len(on["parent"])
        assert n == len(off["parent"]) and n >= 3
        for k in ("parent", "goal", "nrows", "row_offset"):
            assert np.array_equal(on[k], off[k]), k
        assert np.array_equal(_bits(on["state"]), _bits(off["state"]))
        assert np.array_equal(on["costE"].view(np.uint32), off["costE"].view(np.uint32))
        # the kept nodes form a chain whose costS accumulates the rows' terms: equal up to the first node with a
        # row below clear_max, larger from the first node with a row close enough for float32 to see its term
        rows = pl.rows(0, pl.size()[1])
        c = clear_ref.clearance(rows, g, TREE_CLEAR_MAX)
        low = [bool((c[int(on["row_offset"][i]):int(on["row_offset"][i]) + int(on["nrows"][i])] < TREE_CLEAR_MAX).any())
               for i in range(n)]
        near = [bool((c[int(on["row_offset"][i]):int(on["row_offset"][i]) + int(on["nrows"][i])] < 1.5).any())
                for i in range(n)]
        assert any(near) and not all(low)
        first_low, first_near = low.index(True), near.index(True)
        print(f"{n} kept nodes, first with a row below clear_max {first_low}, first with a row within 1.5 m {first_near}")
        assert np.array_equal(on["costS"][:first_low].view(np.uint32), off["costS"][:first_low].view(np.uint32))
        assert (on["costS"] >= off["costS"]).all() and (on["costS"][first_near:] > off["costS"][first_near:]).all()
        # and off again: the tree of the first re-init, byte for byte
        pl.path_load(hdr, prow)
        pl.set_occupancy_clearance(0.0)
        assert pl.tree_init_from_path(car) == abi.REINIT_KEPT
        assert bytes(pl.nodes_raw()) == off_raw
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 6. the point of it
def test_the_committed_path_keeps_more_clearance():
    """The gap scene of tests/test_native_occ_plan.py with the gap widened from [-3, 3) to [-3, 6), one query of 256
    samples x 6 rounds, Wcost[2] = 1000 against the other weights' 10, 5, 4, 1.  Seeds 11, 12, 13.

    Why widened: the car and the goal lie on y = 0, the middle of the symmetric gap, so the straight path the other
    weights prefer is already the clearest one through it and the scene cannot show a preference (measured: the same
    path on and off for all three seeds).  With the upper edge at 6 the straight path still passes 3 m from the lower
    edge, and a path that swings up keeps more clearance."""
    from test_native_occ_plan import _wall
    x0, y0, res, cells, inflate = _wall(16.0)
    cy = y0 + (np.arange(cells.shape[0]) + 0.5) * res
    cells[(cy >= 3.0) & (cy < 6.0), :] = 0
    g = occ_ref.Grid(x0, y0, res, cells, inflate)
    CLEAR_MAX, B, ROUNDS = 3.0, 256, 6

    def mean_clearance(seed, clear_max):
        base = clrrt.default_params(v0=0.0, goal=(40.0, 0.0, 0.0, 0.0), vmax=5.0, collision_mode=OCC)
        base.Wcost[2] = 1000.0
        base.ref_res = max(abs(1.0) * base.ref_int, base.ref_mindist)
        pl = _planner(base, max_nodes=1 << 16, max_rows=1 << 21, max_batch=B, max_obstacles=16)
        try:
            pl.set_obstacles(np.zeros((0, 7)))
            _set_grid(pl, g)
            pl.set_occupancy_clearance(clear_max)
            pl.tree_init_from_path([0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
            pl.expand(clrrt.Rng(seed), n_iters=B * ROUNDS, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
            ids, _, _ = pl.extract_best_path()
            assert len(ids) > 0, seed
            pl.path_commit(ids)
            _, rows = pl.path_download()
            return float(clear_ref.clearance(rows, g, CLEAR_MAX).mean()), list(ids)
        finally:
            pl.close()

    more = 0
    for seed in (11, 12, 13):
        (m_off, ids_off), (m_on, ids_on) = mean_clearance(seed, 0.0), mean_clearance(seed, CLEAR_MAX)
        print(f"seed {seed}: mean clearance along the committed path {m_off:.4f} m off, {m_on:.4f} m on; "
              f"path {ids_off} -> {ids_on}")
        assert m_on >= m_off, seed
        more += m_on > m_off
    assert more >= 1
