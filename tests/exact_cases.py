"""Cases and comparisons of tests/test_exact_rounds.py: EXACT rounds against the oracle's sequential expandTree, one
iteration at a time.

A case is a tuple (start, kind, seed, iters, batch, a, b):
  start "fresh":  the root alone (tree_init); a > 0 sets the query's sortLimit (the window of candidates an iteration
                  tries, 10 in the reference's launch file) on both sides; b unused.
  start "copies": the oracle's tree after `a` iterations (srand(seed)) followed by exact copies of `b` of its nodes
                  (equal keys for every sample: std::sort ties, as tests/test_exact_ties.py builds them), loaded into
                  both sides as node headers.
  start "replan": the oracle's tree after one replanning query of `a` iterations, its best path committed, the pose
                  advanced along it and the tree re-initialised from the committed path (root-pose copies, as
                  tests/test_replan.py builds them); loaded into both sides as node headers, with the second query's
                  car-frame goal and obstacles.
  start "switch": the first `a` nodes of a tree grown on the device in BATCH rounds of 16384 samples (obb200 scene) to
                  more than 12000 nodes -- a tree next to the size at which the EXACT list search changes kernels;
                  the engine loads the grown tree and drops the rest with tree_truncate, the oracle loads the headers.
Both sides then run `iters` iterations from srand(seed + b) / Rng(seed + b): the engine in EXACT rounds of `batch`
samples, the oracle sequentially.  The reference of a case is computed once and never changed (functools.lru_cache;
the arrays are read-only).
"""
import ctypes as C
import functools

import numpy as np

import clrrt
from clrrt import abi, replan, scenes
from oracle_binding import Oracle, nodes_to_numpy

COUNTERS = ("sim_count", "fail_collision", "fail_acclimit", "fail_iterlimit", "rollouts")
ITER_FIELDS = ("nodes",) + COUNTERS  # clrrt_iteration
GOAL_W = (40.0, 0.0, 0.0, 0.0)


def scene(kind):
    if kind == "empty":
        return abi.CLRRT_COLLISION_STUB, None
    if kind == "obb200":
        return abi.CLRRT_COLLISION_OBB, scenes.urban_scene(200)
    if kind == "moving":
        return abi.CLRRT_COLLISION_OBB, scenes.urban_scene(200, 20)
    raise KeyError(kind)


def oracle_steps(o, n):
    """n sequential iterations, one expand(1) each: per iteration the tree-size delta and the counters' deltas,
    int64 [n, 6] in ITER_FIELDS order."""
    rec = np.zeros((n, len(ITER_FIELDS)), dtype=np.int64)
    size, cnt = o.size(), o.counters()
    for i in range(n):
        o.expand(1)
        s2, c2 = o.size(), o.counters()
        rec[i, 0] = s2 - size
        rec[i, 1:] = [c2[k] - cnt[k] for k in COUNTERS]
        size, cnt = s2, c2
    return rec


def _raw_copy(nodes, idx):
    """abi.Node array holding nodes[i] for i in idx."""
    out = (abi.Node * max(1, len(idx)))()
    for k, i in enumerate(idx):
        C.memmove(C.byref(out[k]), C.byref(nodes[i]), C.sizeof(abi.Node))
    return out if len(idx) else (abi.Node * 0)()


@functools.lru_cache(maxsize=None)
def start_tree(case):
    """(params bytes, obstacles or None, node headers to load or None) of a case: host work only."""
    start, kind, seed, iters, batch, a, b = case
    mode, obs = scene(kind)
    p = abi.default_params(collision_mode=mode)
    if start == "fresh":
        if a > 0:
            p.sort_limit = a
        return bytes(p), obs, None
    if start == "switch":
        return bytes(p), obs, _raw_copy(grown_tree(), range(a))
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(seed)
    o.init_tree()
    o.expand(a)
    if start == "copies":
        nodes = o.nodes_raw()
        pick = np.random.default_rng(seed).integers(0, len(nodes), b)
        return bytes(p), obs, _raw_copy(nodes, list(range(len(nodes))) + [int(i) for i in pick])
    if start == "replan":
        make = replan.default_make_params(mode)
        world = np.zeros((0, 7)) if obs is None else obs
        pose = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
        ids = o.extract_best_path()
        assert len(ids) >= 2, "the first query must find a path to re-initialise from"
        o.path_commit(ids)
        o.path_transform(True, pose)
        pn = o.path_nodes()
        rows = np.concatenate([o.path_rows(i) for i in range(len(pn))])
        pose = replan.advance_pose(pose, rows)
        goal_c = replan.goal_in_car_frame(GOAL_W, pose)
        obs_c = replan.obstacles_in_car_frame(world, replan.QUERY_PERIOD, pose)
        p2 = make(pose[4], goal_c)
        o.set_params(p2)
        o.set_obstacles(obs_c)
        o.path_transform(False, pose)
        oc = o.initialize_tree([0.0, 0.0, 0.0, pose[3], pose[4], pose[5]])
        assert oc == abi.REINIT_KEPT, oc
        return bytes(p2), (obs_c if obs is not None else None), o.nodes_raw()
    raise KeyError(start)


SWITCH = 12000  # NN_EXACT_LDS_MAX (clrrt_internal.hpp): tree + round's new nodes up to which EXACT lists stay in LDS
_grown = []


def grown_tree():
    """Node headers of the obb200 tree after BATCH rounds of 16384 samples, grown once per process on the device
    until it passes SWITCH + 512 nodes."""
    if not _grown:
        mode, obs = scene("obb200")
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 17, max_rows=1 << 25,
                           max_batch=16384)
        try:
            pl.set_obstacles(obs)
            pl.tree_init()
            rng = clrrt.Rng(12)
            while pl.size()[0] < SWITCH + 512:
                pl.expand(rng, n_iters=16384, mode=clrrt.CLRRT_MODE_BATCH, batch=16384)
            _grown.append(pl.nodes_raw())
        finally:
            pl.close()
    return _grown[0]


def boundary_start(seed, batch, total, tries=range(0, 8)):
    """A "switch" case of two iterations that stands on the switch.

    Returns (case, d): the tree starts with a = SWITCH + total - d nodes where d = the nodes the oracle's first two
    iterations append from that very tree (found as a fixed point over a: the samples do not depend on a).  A first
    engine round of those two samples that commits both therefore has N + new == SWITCH + total: total 0 puts the
    round exactly at the switch, total 1 starts it below SWITCH and ends above.  Host work on the grown tree."""
    for s in tries:
        a = SWITCH + total - 2
        for _ in range(4):
            case = ("switch", "obb200", seed + s, 2, batch, a, 0)
            o = make_oracle(case)
            d = int(oracle_steps(o, 2)[:, 0].sum())
            if a == SWITCH + total - d:
                break
            a = SWITCH + total - d
        else:
            continue
        if d >= 2 and a < SWITCH:
            return case, d
    raise AssertionError("no seed puts two appending iterations at the switch")


def case_params(case):
    pb, obs, nodes = start_tree(case)
    p = abi.Params()
    C.memmove(C.byref(p), pb, len(pb))
    return p, obs, nodes


def make_oracle(case):
    """The oracle holding the case's start tree, counters zero, rand() seeded for the run."""
    p, obs, nodes = case_params(case)
    o = Oracle(p, obs)
    if nodes is None:
        o.init_tree()
    else:
        o.load_tree(nodes)
    o.reset_counters()
    Oracle.srand(case[2] + case[6])
    return o


def snapshot(o, first_new, rec):
    """What a run is compared by, as read-only data: node headers, the rows of the nodes appended since first_new,
    counters, per-iteration records."""
    nd = nodes_to_numpy(o.nodes_raw())
    rows = [np.ascontiguousarray(o.rows(i)) for i in range(first_new, o.size())]
    for v in list(nd.values()) + rows + [rec]:
        v.setflags(write=False)
    return {"nodes": nd, "rows": rows, "counters": o.counters(), "records": rec, "first_new": first_new}


@functools.lru_cache(maxsize=None)
def reference(case):
    o = make_oracle(case)
    first_new = o.size()
    rec = oracle_steps(o, case[3])
    return snapshot(o, first_new, rec)


def make_planner(case, options=None, max_nodes=1 << 16, max_rows=1 << 22):
    p, obs, nodes = case_params(case)
    pl = clrrt.Planner(p, max_nodes=max_nodes, max_rows=max_rows, max_batch=case[4])
    for k, v in (options or {}).items():
        pl.set_option(k, v)
    if obs is not None:
        pl.set_obstacles(obs)
    if nodes is None:
        pl.tree_init()
    elif case[0] == "switch":
        pl.tree_load(grown_tree())
        pl.tree_truncate(case[5])
    else:
        pl.tree_load(nodes)
    return pl


def run_engine(case, options=None):
    """The case on the engine with the iteration log on: (planner, stats, iteration records [n, 6])."""
    pl = make_planner(case, options)
    pl.iteration_log(True)
    st = pl.expand(clrrt.Rng(case[2] + case[6]), n_iters=case[3], mode=clrrt.CLRRT_MODE_EXACT, batch=case[4])
    return pl, st, records(pl)


def records(pl):
    it = pl.iterations()
    return np.stack([it[f] for f in ITER_FIELDS], axis=1).reshape(-1, len(ITER_FIELDS))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_parity(ref, pl, rec, label, counters=None):
    """Engine == oracle, bit for bit: every node header field both sides carry, the rows of every appended node, the
    counters' totals and every field of every iteration record."""
    on, gn = ref["nodes"], pl.nodes()
    f0 = ref["first_new"]
    n = len(on["parent"])
    assert len(gn["parent"]) == n, (label, "tree size", n, len(gn["parent"]))
    for f in ("parent", "goal"):
        bad = np.flatnonzero(on[f] != gn[f])
        assert bad.size == 0, (label, f, int(bad[0]))
    for f in ("state", "costE", "costS", "ref_front", "ref_back", "ref_vback"):
        bad = np.flatnonzero((_bits(on[f]) != _bits(gn[f])).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (label, f, "first differing node", int(bad[0]))
    assert np.array_equal(on["nrows"][f0:], gn["nrows"][f0:]), (label, "nrows")
    for i in range(f0, n):
        rows = pl.rows(int(gn["row_offset"][i]), int(gn["nrows"][i]))
        assert np.array_equal(_bits(rows), _bits(ref["rows"][i - f0])), (label, "rows of node", i)
    gc = pl.counters() if counters is None else counters
    for k in COUNTERS:
        assert ref["counters"][k] == gc[k], (label, k, ref["counters"][k], gc[k])
    want = ref["records"]
    assert rec.shape == want.shape, (label, "iteration records", rec.shape, want.shape)
    bad = np.flatnonzero((rec != want).any(axis=1))
    assert bad.size == 0, (label, "first differing iteration", int(bad[0]), ITER_FIELDS, want[bad[0]].tolist(),
                           rec[bad[0]].tolist())


def cap_reaching_iterations(case, cap):
    """Iterations of the sequential run that try, before their result, a node appended by one of the two iterations
    before them whose rollout for the sample runs more than `cap` steps: in EXACT rounds that rollout is a fix-up
    rollout (the node is new in the round unless a round boundary falls between) which a cap of `cap` steps stops
    undecided.  Host work only."""
    p, obs, nodes = case_params(case)
    o = make_oracle(case)
    smp = clrrt.Rng(case[2] + case[6]).draw_samples(p, case[3])
    sizes = [o.size()]
    hits = []
    for j in range(case[3]):
        s = smp[j]
        recent = sizes[max(0, j - 2)]
        ids, _ = o.sort_nodes(s.x, s.y, s.explore)
        for c in ids[:p.sort_limit]:
            r = o.simulate(c, 0, s.x, s.y)
            if r["outcome"] in (abi.ROLL_END, abi.ROLL_GOAL):
                break
            if c >= recent and r["nrows"] - 1 > cap:
                hits.append(j)
        o.expand(1)
        sizes.append(o.size())
    return hits
