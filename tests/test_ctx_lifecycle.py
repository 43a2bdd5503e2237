"""A context's whole life, three times in one process -- GPU.

Each cycle creates a context with small capacities (max_batch 256, max_nodes 32768, nn_walk_min 64 so the walk sets
allocate), touches every lazily allocated buffer group and drives the grow sites across a capacity increase after the
old buffer has been used, then destroys it:

  EXACT rounds with fix-ups (fix_*), a lag-1 and a lag-2 BATCH expansion (the list sets' third, the walk sets, with
  nn_delta_verify the appended-node walk's set and the brute force's buffers), defer_steps 64 then 16 (the rings and
  the commit buffers re-grow), rows_deferred 0 and then a smaller sim_dt (the row slots, re-grown), clrrt_nn_range and
  clrrt_nn_merge with 2 then 4 parts, 8 then 200 obstacles (the cull grid), an occupancy grid of 64 x 64 then
  256 x 256 cells with the clearance on, off and on, the best path and a committed path of 2 then more nodes, and a
  one-rank sharded expansion over the in-process transport (option shard_hook_world1).

Every call returns OK; the three cycles give identical trees, lists, fields and paths (a re-created context carries
nothing over); and each cycle's lag-2 and deferred trees are those of a fresh context that runs that query alone (a
buffer re-grown in mid-life changes nothing).  Re-growth that other tests already cross, at their sizes:
test_nn_partition (clrrt_nn_merge's inputs, 1 -> 2 -> 3 -> 8 parts on one context), test_replan (the committed path's
buffers and the cull grid over the replanning queries), test_clear_gpu (the field freed and re-baked), test_occ_gpu
(grids replaced on one context), test_dist_gpu / test_native_xchg (the sharded commit's record buffers, which need
more than 2048 records in one round to grow)."""
import ctypes as C

import numpy as np
import pytest

import clrrt
from clrrt import abi, scenes
from clrrt import dist as cdist

pytestmark = pytest.mark.gpu

B, NODES, ROWS = 256, 1 << 15, 1 << 22
SEED = 12
OBB, OCC = abi.CLRRT_COLLISION_OBB, abi.CLRRT_COLLISION_OCC
BATCH, EXACT = clrrt.CLRRT_MODE_BATCH, clrrt.CLRRT_MODE_EXACT
# the three queries a fresh context repeats alone: (options, rounds)
LAG2 = (dict(nn_lag=2, nn_delta_verify=1, defer_steps=0), 8)
DEF64 = (dict(nn_lag=2, nn_delta_verify=0, defer_steps=64), 6)
DEF16 = (dict(nn_lag=2, nn_delta_verify=0, defer_steps=16), 6)


def _planner():
    pl = clrrt.Planner(clrrt.default_params(collision_mode=OBB), max_nodes=NODES, max_rows=ROWS, max_batch=B)
    pl.set_option("nn_walk_min", 64)
    return pl


def _tree(pl):
    n, nr = pl.size()
    return n, bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes()


def _query(pl, opts, rounds, mode=BATCH):
    """One query from a fresh root under `opts`; the tree it grew."""
    for k, v in opts.items():
        pl.set_option(k, v)
    pl.tree_init()
    st = pl.expand(clrrt.Rng(SEED), n_iters=B * rounds, mode=mode, batch=B)
    assert mode != BATCH or st["rounds"] == rounds, st
    return _tree(pl)


def _grid(w):
    """w x w cells of 0.25 m ahead of the car, a block of occupied cells in the far corner."""
    cells = np.zeros((w, w), dtype=np.uint8)
    cells[w - w // 8:, w - w // 8:] = 1
    return dict(x0=5.0, y0=-w * 0.125, res=0.25, cells2d=cells)


def _chain(parent, leaf):
    ids = [leaf]
    while parent[ids[-1]] >= 0:
        ids.append(int(parent[ids[-1]]))
    return ids[::-1]


def _cycle():
    out = {}
    pl = _planner()
    try:
        # 8 obstacles, EXACT rounds with fix-ups; then 200 obstacles (the grid buffer grows after it was used)
        pl.set_obstacles(scenes.urban_scene(8))
        pl.set_option("exact_fixup", 1)
        out["exact8"] = _query(pl, {}, 1, mode=EXACT)
        assert pl.exact_stats()["rounds"] > 0
        pl.set_obstacles(scenes.urban_scene(200))
        out["exact200"] = _query(pl, {}, 1, mode=EXACT)
        # lag-1, then lag-2 BATCH rounds (the appended-node walk checked against the brute force)
        out["lag1"] = _query(pl, dict(nn_lag=1), 6)
        out["lag2"] = _query(pl, *LAG2)
        d = pl.debug_counters()
        assert d[38] > 0 and d[39] == 0, (d[38], d[39])
        # deferred samples: T = 64, then 16 on the same context (more ring slots, more commit views)
        out["def64"] = _query(pl, *DEF64)
        out["def16"] = _query(pl, *DEF16)
        # rows stored by the speculative rollouts (the row slots), then longer slots for a smaller sim_dt
        out["slots"] = _query(pl, dict(defer_steps=0, rows_deferred=0, nn_lag=1), 4)
        p = clrrt.default_params(collision_mode=OBB)
        p.sim_dt = 0.02
        pl.set_params(p)
        out["slots_dt"] = _query(pl, {}, 2)
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        pl.set_option("rows_deferred", 1)
        # tree-partitioned search over the tree the lag-1 query leaves: 2 parts, then 4
        tree = _query(pl, {}, 6)
        assert tree == out["lag1"]
        N = tree[0]
        assert N > 4 * 64
        smp = clrrt.Rng(77).draw_samples(pl.params, 200)
        for parts in (2, 4):
            lists = [pl.nn_range(smp, *cdist.node_range(N, parts, r)) for r in range(parts)]
            ids, keys, cnt = pl.nn_merge(*[np.stack([q[i] for q in lists]) for i in range(3)])
            out[f"merge{parts}"] = (ids.tobytes(), keys.tobytes(), cnt.tobytes())
        assert out["merge2"] == out["merge4"]
        # best path (none need exist) and the committed path: 2 nodes, then the deepest chain
        best, _, ngoal = pl.extract_best_path()
        par = pl.nodes()["parent"]
        depth = np.zeros(N, dtype=np.int64)
        for i in range(1, N):
            depth[i] = depth[par[i]] + 1  # parents precede their children
        long_chain = _chain(par, int(np.argmax(depth)))
        assert len(long_chain) > 4
        paths = []
        for ids in (long_chain[:2], long_chain):
            assert pl.path_commit(ids) == 0
            hdr, rows = pl.path_download()
            paths.append((bytes(hdr), rows.tobytes()))
        out["paths"] = (best, ngoal, paths)
        # occupancy: 64 x 64 then 256 x 256 cells, the clearance on, off and on; a mode-2 query over the last
        pl.set_occupancy_clearance(3.0)
        pl.set_occupancy(**_grid(64))
        f64 = pl.occupancy_field().tobytes()
        pl.set_occupancy(**_grid(256))
        f256 = pl.occupancy_field().tobytes()
        assert pl.occupancy_clearance_info()["baked"]
        pl.set_occupancy_clearance(0.0)
        assert not pl.occupancy_clearance_info()["baked"]
        pl.set_occupancy_clearance(3.0)
        assert pl.occupancy_field().tobytes() == f256
        pl.set_params(clrrt.default_params(collision_mode=OCC))
        out["occ"] = (f64, f256, _query(pl, {}, 3))
        pl.set_params(clrrt.default_params(collision_mode=OBB))
        pl.set_occupancy(cells2d=None)
        # one rank's sharded rounds through the native hook over the in-process transport
        X = cdist.xchg_lib()
        g, x = C.c_void_p(), C.c_void_p()
        assert X.clrrt_xchg_group_create(1, 10000, C.byref(g)) == 0
        try:
            assert X.clrrt_xchg_create_local(g, 0, 0, cdist.exchange_capacity(B), B + 64, C.byref(x)) == 0, \
                X.clrrt_xchg_last_error()
            try:
                pl.set_option("shard_hook_world1", 1)
                assert X.clrrt_xchg_attach(x, pl.h) == 0, X.clrrt_xchg_last_error()
                out["shard"] = _query(pl, {}, 4)
                st = (C.c_int64 * 8)()
                assert X.clrrt_xchg_stats(x, st) == 0 and st[0] >= 4  # an exchange per round (and the closing one)
                pl.set_shards(0, 1)
            finally:
                X.clrrt_xchg_destroy(x)
        finally:
            X.clrrt_xchg_group_destroy(g)
    finally:
        pl.close()
    return out


def _alone(opts, rounds):
    """The query on a fresh context that runs nothing else (200 obstacles): no buffer of it ever re-grew."""
    pl = _planner()
    try:
        pl.set_obstacles(scenes.urban_scene(200))
        return _query(pl, opts, rounds)
    finally:
        pl.close()


def test_three_lives_of_a_context():
    lives = [_cycle() for _ in range(3)]
    first = lives[0]
    print({k: v[0] for k, v in first.items() if k not in ("merge2", "merge4", "paths", "occ")},
          "occ tree", first["occ"][2][0], "path nodes", [len(p[0]) // 160 for p in first["paths"][2]])
    for k in ("exact8", "exact200", "lag1", "lag2", "def64", "def16", "slots", "slots_dt", "shard"):
        assert first[k][0] > B // 2, (k, first[k][0])  # the queries grew trees
    assert first["exact8"] != first["exact200"]  # the second obstacle set is the one in force
    for life in lives[1:]:
        assert life.keys() == first.keys()
        for k in first:
            assert life[k] == first[k], k
    for life in lives:
        assert life["lag2"] == _fresh("lag2")
        assert life["def64"] == _fresh("def64")
        assert life["def16"] == _fresh("def16")


_alone_trees = {}


def _fresh(name):
    if name not in _alone_trees:
        _alone_trees[name] = _alone(*{"lag2": LAG2, "def64": DEF64, "def16": DEF16}[name])
    return _alone_trees[name]
