"""Occupancy-grid collision mode (CLRRT_COLLISION_OCC = 2: the static grid of clrrt_set_occupancy, then the obstacle
list as mode 1) -- GPU.

The oracle has no grid mode; the references are numpy (tests/occ_ref.py) and the engine's own stub and OBB modes,
which the oracle pins.  The state sets and grids come from tests/occ_cases.py; tests/test_occ_host.py checks their
input conditions on the CPU (hit shares, borderline shares).  A state whose decision margin is within 1e-9 of 0
(occ_ref.BORDER) is borderline -- the device's cosine may differ from numpy's by an ulp -- and is the only kind of
state a test here skips.
"""
import ctypes as C

import numpy as np
import pytest

import clrrt
import occ_cases
import occ_ref
from clrrt import abi, scenes
from test_gpu_parity import _compare_trees, _nn_strategy

pytestmark = pytest.mark.gpu

OCC, OBB, STUB = abi.CLRRT_COLLISION_OCC, abi.CLRRT_COLLISION_OBB, abi.CLRRT_COLLISION_STUB
PLACE = {"lds": abi.OCC_LDS, "global": abi.OCC_GLOBAL}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _set_grid(pl, g):
    pl.set_occupancy(g.x0, g.y0, g.res, g.cells, g.inflate)


_cases = {}


def _case(name):
    """(grid, placement, states, hit, borderline) of a grid: the numpy reference, computed once."""
    if name not in _cases:
        g, place = occ_cases.grids()[name]
        st = occ_cases.states(name, g)
        m = occ_ref.margin(st, g)
        _cases[name] = (g, place, st, m <= 0.0, np.abs(m) <= occ_ref.BORDER)
    return _cases[name]


# ------------------------------------------------------------------------------------------------ 1. decision
@pytest.mark.parametrize("name", list(occ_cases.grids()))
def test_decision_matches_numpy(name):
    g, place, st, hit, skip = _case(name)
    keep = ~skip
    print(f"{name}: {hit.sum()} of {len(st)} states hit, {skip.sum()} borderline (skipped)")
    pl = clrrt.Planner(clrrt.default_params(collision_mode=OCC), max_nodes=1 << 10, max_rows=1 << 14, max_batch=64)
    try:
        _set_grid(pl, g)
        info = pl.occupancy_info()
        assert (info["w"], info["h"]) == (g.cells.shape[1], g.cells.shape[0])
        assert info["occupied"] == int(np.count_nonzero(g.cells))
        assert info["placement"] == PLACE[place], info
        # no obstacle list: 0 on a hit, else mode 1's value without obstacles
        want = np.where(hit, 0.0, 10000.0)
        got = pl.check_obs_distance(st)
        assert np.array_equal(got[keep], want[keep]), np.nonzero(keep & (got != want))[0][:8]
        for path in (pl.COLL_EXHAUSTIVE, pl.COLL_LANE, pl.COLL_LANE_NOGRID):
            d, t = pl.selftest_collision(path, st)
            assert np.array_equal(d[keep], want[keep]), (path, np.nonzero(keep & (d != want))[0][:8])
            assert not t.any()
        # with the obstacle list: 0 on a grid hit (no box test made or counted), else mode 1's value, bit for bit
        pl.set_obstacles(scenes.urban_scene(200, 20))
        assert pl.occupancy_info()["placement"] == PLACE[place]
        ref = {}
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        assert pl.grid_info(lists=False)["coop"]
        ref["dist"] = pl.check_obs_distance(st)
        paths = (pl.COLL_EXHAUSTIVE, pl.COLL_LANE, pl.COLL_LANE_NOGRID, pl.COLL_COOP)
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
        # idle lanes of the cooperative path stay idle
        act = (np.arange(len(st)) % 3 != 0).astype(np.int32)
        d2, t2 = pl.selftest_collision(pl.COLL_COOP, st, act)
        d1, t1 = ref[pl.COLL_COOP]
        on = keep & (act != 0)
        assert np.array_equal(d2[act == 0], np.full((act == 0).sum(), -1.0)) and not t2[act == 0].any()
        assert np.array_equal(_bits(d2[on]), _bits(np.where(hit, 0.0, d1)[on]))
    finally:
        pl.close()


def test_mode_2_without_a_grid_is_mode_1_and_the_grid_is_ignored_elsewhere():
    g, _, st, hit, skip = _case("full_row")
    pl = clrrt.Planner(clrrt.default_params(collision_mode=OBB), max_nodes=1 << 10, max_rows=1 << 14, max_batch=64)
    try:
        pl.set_obstacles(scenes.urban_scene(200, 20))
        ref = pl.check_obs_distance(st)
        _set_grid(pl, g)  # legal in any mode, read only in mode 2
        assert np.array_equal(_bits(pl.check_obs_distance(st)), _bits(ref))
        pl.set_params(clrrt.default_params(collision_mode=STUB))
        assert np.array_equal(pl.check_obs_distance(st), np.full(len(st), 100.0))
        pl.set_params(clrrt.default_params(collision_mode=OCC))
        assert (pl.check_obs_distance(st)[hit & ~skip] == 0).all()
        pl.set_occupancy(cells2d=None)  # cleared: mode 2 is mode 1
        assert pl.occupancy_info()["w"] == 0 and pl.occupancy_info()["placement"] == abi.OCC_NONE
        assert np.array_equal(_bits(pl.check_obs_distance(st)), _bits(ref))
        d, t = pl.selftest_collision(pl.COLL_COOP, st)
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        d1, t1 = pl.selftest_collision(pl.COLL_COOP, st)
        assert np.array_equal(_bits(d), _bits(d1)) and np.array_equal(t, t1)
    finally:
        pl.close()


def test_set_occupancy_validates_its_input():
    pl = clrrt.Planner(clrrt.default_params(collision_mode=OCC), max_nodes=1 << 10, max_rows=1 << 14, max_batch=64)
    try:
        cells = np.zeros(64, np.uint8)
        ptr = C.c_void_p(cells.ctypes.data)

        def rc(x0=0.0, y0=0.0, res=0.5, inflate=0.0, w=8, h=8, p=ptr):
            o = abi.Occupancy(x0, y0, res, inflate, w, h)
            r = pl.L.clrrt_set_occupancy(pl.h, C.byref(o), p)
            return r, pl.L.clrrt_last_error(pl.h).decode()

        assert rc()[0] == 0 and pl.occupancy_info()["w"] == 8
        for kw, word in ((dict(w=-1), "w"), (dict(w=2049), "w"), (dict(h=0), "h"), (dict(h=4096), "h"),
                         (dict(x0=np.nan), "x0"), (dict(y0=np.inf), "y0"), (dict(res=0.0), "res"),
                         (dict(res=-1.0), "res"), (dict(res=np.nan), "res"), (dict(inflate=-0.1), "inflate"),
                         (dict(inflate=np.nan), "inflate"), (dict(p=None), "cells"),
                         (dict(x0=1e12, res=1e-3), "res")):
            r, msg = rc(**kw)
            assert r == -1 and word in msg.split("set_occupancy:")[1].split()[0:2], (kw, r, msg)
        assert pl.occupancy_info()["w"] == 8  # a refused call leaves the grid as it was
        assert rc(w=0)[0] == 0 and pl.occupancy_info()["w"] == 0  # w == 0 clears
        big = np.zeros(2048 * 2048, np.uint8)
        assert rc(w=2048, h=2048, p=C.c_void_p(big.ctypes.data))[0] == 0
        assert rc(w=2048, h=2048 + 1, p=C.c_void_p(big.ctypes.data))[0] == -1
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 2. rollouts
def test_rollouts_end_at_the_first_hitting_row():
    g = occ_cases.wall_with_gap()
    jobs = occ_cases.rollout_jobs()
    pl = clrrt.Planner(clrrt.default_params(collision_mode=STUB), max_nodes=1 << 10, max_rows=1 << 14, max_batch=512)
    try:
        pl.tree_init()
        ref = pl.simulate_batch(jobs, rows=True)
        pl.set_params(clrrt.default_params(collision_mode=OCC))
        _set_grid(pl, g)
        assert pl.occupancy_info()["placement"] == abi.OCC_LDS
        got = pl.simulate_batch(jobs, rows=True)
        n_hit = n_free = n_skip = 0
        for j, (a, b) in enumerate(zip(ref, got)):
            k, border = occ_ref.first_hit_row(a["rows"], g)
            if border:
                n_skip += 1
                continue
            if k < 0:
                n_free += 1
                assert (b["outcome"], b["nrows"], b["ref_n"]) == (a["outcome"], a["nrows"], a["ref_n"]), j
                assert _bits([b["costE"], b["costS"]]).tolist() == _bits([a["costE"], a["costS"]]).tolist(), j
                assert np.array_equal(_bits(b["rows"]), _bits(a["rows"])), j
                assert np.array_equal(_bits(b["final"]), _bits(a["final"])), j
            else:
                n_hit += 1
                assert b["outcome"] == abi.ROLL_COLLISION and b["nrows"] == k + 1, (j, k, b["outcome"], b["nrows"])
                assert np.array_equal(_bits(b["rows"][:k]), _bits(a["rows"][:k])), j
        print(f"rollouts: {n_hit} end at the wall, {n_free} free, {n_skip} borderline")
        assert n_hit >= 100 and n_free >= 100 and n_skip <= 2
    finally:
        pl.close()


# ------------------------------------------------------------------------------------------------ 3. all-free grid
def _grow(mode, variant, obs, grid=None, batch=256, rounds=4, seed=6):
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 21, max_batch=batch)
    for k, v in variant.get("opts", {}).items():
        pl.set_option(k, v)
    _nn_strategy(pl, variant["nn"])
    if obs is not None:
        pl.set_obstacles(obs)
    if grid is not None:
        _set_grid(pl, grid)
    pl.tree_init()
    if variant.get("exact"):
        st = pl.expand(clrrt.Rng(seed), n_iters=variant["exact"], mode=clrrt.CLRRT_MODE_EXACT, batch=batch)
        assert st["iterations"] == variant["exact"]
    else:
        st = pl.expand(clrrt.Rng(seed), n_iters=batch * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
        assert st["rounds"] == rounds, st
    return pl


def _same_tree(a, b, label):
    """Planner b's tree is planner a's: headers, costs, rows and the five counters."""
    an, bn, bad = _compare_trees(a, b, label)
    assert bad is None and len(an["parent"]) == len(bn["parent"])
    for k in ("costE", "costS"):
        assert np.array_equal(an[k].view(np.uint32), bn[k].view(np.uint32)), k
    for k in ("ref_front", "ref_back", "ref_vback", "ang_par"):
        assert np.array_equal(_bits(an[k]), _bits(bn[k])), k
    for i in range(1, len(an["parent"])):
        ra = a.rows(int(an["row_offset"][i]), int(an["nrows"][i]))
        rb = b.rows(int(bn["row_offset"][i]), int(bn["nrows"][i]))
        assert np.array_equal(_bits(ra), _bits(rb)), i
    assert a.counters() == b.counters(), (a.counters(), b.counters())
    return len(an["parent"])


# The box-test work counter counts the tests of every simulated step, those of speculative candidates included.  The
# persistent rollout kernel abandons a candidate once an earlier one of its sample has succeeded, at a step that
# depends on how the waves were scheduled, so under it the counter is not reproducible from run to run in mode 1
# itself (the tree, the rows and the five counters are).  With one lane per candidate (roll_persistent 0) every
# candidate runs to its end: there the counter is compared strictly; under the persistent kernel it is compared
# whenever two mode-1 runs agree with each other, and all three figures are printed.
ALL_FREE = [dict(nn="brute", opts=dict(defer_steps=0)), dict(nn="walk", opts=dict(defer_steps=32, nn_lag=2)),
            dict(nn="brute", exact=300), dict(nn="brute", opts=dict(defer_steps=0, roll_persistent=0), strict=True)]


@pytest.mark.parametrize("variant", ALL_FREE, ids=["batch_T0_brute", "batch_T32_walk_lag2", "exact_300",
                                                   "batch_T0_brute_lane_per_candidate"])
def test_all_free_grid_is_mode_1(variant):
    obs = scenes.urban_scene(200, 20)
    free = occ_ref.Grid(0.0, -24.0, 0.2, np.zeros((240, 330), np.uint8), occ_ref.default_inflate(0.2))
    a = _grow(OBB, variant, obs)
    a2 = _grow(OBB, variant, obs)
    b = _grow(OCC, variant, obs, free)
    try:
        assert b.occupancy_info()["w"] == 330 and b.occupancy_info()["occupied"] == 0
        n = _same_tree(a, b, "all-free grid")
        assert n > 50
        assert b.debug_counters()[3] == 0  # no step took the exact scan
        wa, wa2, wb = (p.work_counters()["box_tests"] for p in (a, a2, b))
        print(f"box tests: mode 1 {wa}, mode 1 again {wa2}, mode 2 with an all-free grid {wb}")
        if variant.get("strict"):
            assert wa == wa2 == wb
        else:
            assert wb == wa or wa != wa2
    finally:
        a.close()
        a2.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 4. round 1
def _first_round(mode, grid, seed):
    import torch
    B = 256
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 12, max_rows=1 << 20, max_batch=B)
    if grid is not None:
        _set_grid(pl, grid)
    pl.tree_init()
    smp = clrrt.Rng(seed).draw_samples(pl.params, B)
    out = torch.empty((2 * B, 160), dtype=torch.uint8, device="cuda")
    n = pl.round_eval(smp, out.data_ptr())
    pl.round_commit(out.data_ptr(), n, 0, n)
    pl.rows_flush()
    nodes = pl.nodes()
    assert len(nodes["parent"]) == n + 1
    rows = [pl.rows(int(nodes["row_offset"][i]), int(nodes["nrows"][i])) for i in range(n + 1)]
    pl.close()
    return nodes, rows


def test_first_round_is_the_stub_round_filtered():
    g = occ_cases.wall_with_gap()
    for seed in range(11, 40):  # the first seed none of whose rows is borderline (decided by numpy alone)
        sn, srows = _first_round(STUB, None, seed)
        ms = [occ_ref.margin(r[1:], g) for r in srows[1:]]
        if not any((np.abs(m) <= occ_ref.BORDER).any() for m in ms):
            break
    else:
        raise AssertionError("no seed without a borderline row")
    hit = [False] + [bool((m <= 0.0).any()) for m in ms]
    n = len(sn["parent"])
    # from the root every sample has one candidate: a regular node (parent 0) and, right behind it, its goal-biased
    # follow-up (parent = the regular node).  A follow-up goes with its regular node, or alone when only its rows hit.
    keep, new_id = [], {0: 0}
    for i in range(1, n):
        par = int(sn["parent"][i])
        assert par == 0 or par == i - 1
        if hit[i] or par not in new_id:
            continue
        new_id[i] = len(new_id)
        keep.append(i)
    on, orows = _first_round(OCC, g, seed)
    print(f"seed {seed}: stub round {n - 1} records, {sum(hit)} with a hitting row, mode 2 {len(on['parent']) - 1}")
    assert sum(hit) >= 20 and len(keep) >= 20 and any(int(sn["parent"][i]) != 0 for i in keep)
    assert any(hit[i] and int(sn["parent"][i]) != 0 and not hit[i - 1] for i in range(1, n))  # a follow-up dropped alone
    assert len(on["parent"]) == len(keep) + 1
    for q, i in enumerate(keep, start=1):
        assert int(on["parent"][q]) == new_id[int(sn["parent"][i])], (q, i)
        for k in ("state", "ref_front", "ref_back", "ref_vback", "ang_par"):
            assert np.array_equal(_bits(on[k][q]), _bits(sn[k][i])), (k, q, i)
        for k in ("costE", "costS", "goal", "nrows"):
            assert on[k][q] == sn[k][i], (k, q, i)
        assert np.array_equal(_bits(orows[q]), _bits(srows[i])), (q, i)


# ------------------------------------------------------------------------------------------------ 5. expansions
def _cfg3_grid():
    obs = scenes.urban_scene(200, 20)
    x0, y0, res, w, h = 0.0, -26.0, 0.2, 330, 260
    cells = scenes.rasterize(obs, x0, y0, res, w, h)
    return obs[200:], occ_ref.Grid(x0, y0, res, cells, occ_ref.default_inflate(res))


# The tree of a BATCH expansion depends on defer_steps by design (a deferred sample commits in a later round; the
# oracle's expand_batch takes the same parameter), so pipelines are compared within one defer_steps: the two with
# T 0 with each other, and the T 32 lag-2 walk with the T 32 lag-1 brute force.
PIPELINES = [dict(nn="brute", opts=dict(defer_steps=0)), dict(nn="walk_split", opts=dict(defer_steps=0, nn_lag=1)),
             dict(nn="walk", opts=dict(defer_steps=32, nn_lag=2)), dict(nn="brute", opts=dict(defer_steps=32, nn_lag=1))]


def test_whole_expansions_keep_clear_of_the_grid():
    movers, g = _cfg3_grid()
    assert np.count_nonzero(g.cells) > 5000
    pls = [_grow(OCC, v, movers, g, rounds=6) for v in PIPELINES]
    try:
        a = pls[0]
        nodes = a.nodes()
        n = len(nodes["parent"])
        assert n > 100 and a.counters()["fail_collision"] > 100
        for p in (pls[0], pls[2]):
            nodes = p.nodes()
            n = len(nodes["parent"])
            rows = np.concatenate([p.rows(int(nodes["row_offset"][i]), int(nodes["nrows"][i]))[1:]
                                   for i in range(1, n)])
            m = occ_ref.margin(rows, g)
            print(f"{n} nodes, {len(rows)} rows, smallest margin {m.min():.3e}, exact scans "
                  f"{p.debug_counters()[3]} of {p.work_counters()['steps']} steps")
            assert not (m <= -occ_ref.BORDER).any()  # no row of any node hits (a borderline one may fall either way)
            assert p.debug_counters()[3] > 0
        _same_tree(pls[0], pls[1], "T 0: brute force | every sample through the overflow split, lag 1")
        _same_tree(pls[2], pls[3], "T 32: walk, lag 2 | brute force, lag 1")
        # the grid set, cleared and set again reproduces the tree
        b = pls[1]
        b.set_occupancy(cells2d=None)
        _set_grid(b, g)
        b.tree_init()
        b.reset_counters()
        st = b.expand(clrrt.Rng(6), n_iters=256 * 6, mode=clrrt.CLRRT_MODE_BATCH, batch=256)
        assert st["rounds"] == 6
        _same_tree(a, b, "set, cleared, set again")
    finally:
        for p in pls:
            p.close()


# ------------------------------------------------------------------------------------------------ 6. re-init
def test_reinit_checks_the_path_rows_against_the_grid():
    def planner(mode):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 22,
                           max_batch=256)
        pl.tree_init()
        pl.expand(clrrt.Rng(4), n_iters=256 * 6, mode=clrrt.CLRRT_MODE_BATCH, batch=256)  # an empty world
        ids, _, ngoal = pl.extract_best_path()
        assert ngoal > 0 and len(ids) >= 3
        pl.path_commit(ids)
        return pl, ids

    a, ids = planner(OBB)
    b, ids_b = planner(OCC)
    try:
        assert ids == ids_b
        hdr, prow = a.path_download()
        third = hdr[2]  # the path's third node
        seg = prow[third.row_offset:third.row_offset + third.nrows]
        x0, y0, res = -5.0, -15.0, 0.25
        w, h = 240, 120
        # the cell under a row of that node's, chosen with numpy so that no row of the path lies within 1 cm of
        # either decision boundary (the grid's with inflate 0, and the 2 mm box's, whose half extent is 1 mm)
        for r in seg[len(seg) // 2:]:
            c, s = np.cos(r[2]), np.sin(r[2])
            i = int(np.floor((r[0] + occ_ref.OFF * c - x0) / res))
            j = int(np.floor((r[1] + occ_ref.OFF * s - y0) / res))
            cells = np.zeros((h, w), np.uint8)
            cells[j, i] = 1
            g = occ_ref.Grid(x0, y0, res, cells, 0.0)
            m = occ_ref.margin(prow, g)
            if (np.abs(m) > 0.011).all() and (m <= 0).any():
                break
        else:
            raise AssertionError("no cell with every path row 1 cm clear of the boundary")
        cx, cy = x0 + (i + 0.5) * res, y0 + (j + 0.5) * res
        car = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        a.set_obstacles(np.array([[cx, cy, 0.0, 0.004, 0.004, 0.0, 0.0]]))
        _set_grid(b, g)
        oa, ob = a.tree_init_from_path(car), b.tree_init_from_path(car)
        assert oa == ob == abi.REINIT_COLLISION
        assert bytes(a.nodes_raw()) == bytes(b.nodes_raw()) and a.size() == b.size() == (1, 1)
        # the cell cleared again: the path's survivors, as mode 1 keeps them in the empty world
        a.set_obstacles(np.zeros((0, 7)))
        _set_grid(b, g._replace(cells=np.zeros((h, w), np.uint8)))
        a.path_load(hdr, prow)
        b.path_load(hdr, prow)
        oa, ob = a.tree_init_from_path(car), b.tree_init_from_path(car)
        assert oa == ob == abi.REINIT_KEPT
        assert bytes(a.nodes_raw()) == bytes(b.nodes_raw()) and a.size() == b.size() and a.size()[0] > 1
        na, nr = a.size()
        assert np.array_equal(_bits(a.rows(0, nr)), _bits(b.rows(0, nr)))
    finally:
        a.close()
        b.close()
