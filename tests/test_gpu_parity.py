"""Parity of the HIP path (libclrrt through its C-ABI) with the CPU oracle on the same inputs.

Tolerance: none.  Every libm call on the rollout and key path is glibc's own algorithm restated for the
device (clrrt_glibc.hpp, clrrt_glibcf.hpp; checked against the host libm exhaustively for the float
functions), so rollouts (outcome, step count, every FP64 state bit, costs, rows), candidate lists and
FP32 Dubins keys must equal the oracle's bit for bit.  (The north star allows "a stated float
tolerance"; the stated tolerance is 0 ulp.)  The remaining GPU-math calls — double atan2 in
feasibleNode's angle test and exp of the unused W2 obstacle term — cannot change a result except on a
~1e-16 rad band around the pi/4 threshold.
"""
import numpy as np
import pytest

import clrrt
from clrrt import abi, scenes
from nn_strategies import nn_strategy as _nn_strategy  # noqa: F401 (other test modules import it from here)
from oracle_binding import Oracle

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-9  # kept for the diagnostics printed on a failure; the asserts are bitwise


def _close(a, b, rtol=RTOL, atol=ATOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= atol + rtol * np.abs(b)) or np.array_equal(a, b, equal_nan=True)


def _scene(kind):
    if kind == "empty":
        return abi.CLRRT_COLLISION_STUB, None
    if kind == "obb200":
        return abi.CLRRT_COLLISION_OBB, scenes.urban_scene(200)
    if kind == "moving":
        return abi.CLRRT_COLLISION_OBB, scenes.urban_scene(200, 20)
    raise KeyError(kind)


def _pair(kind, seed=1, iters=40):
    """Oracle grown `iters` iterations + a GPU planner holding the same tree."""
    mode, obs = _scene(kind)
    q = abi.default_params(collision_mode=mode)
    o = Oracle(q, obs)
    Oracle.srand(seed)
    o.init_tree()
    o.expand(iters)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 20,
                       max_batch=2048)
    if obs is not None:
        pl.set_obstacles(obs)
    pl.tree_load(o.nodes_raw())
    return o, pl


@pytest.mark.parametrize("kind", ["empty", "obb200", "moving"])
def test_rollout_parity(kind):
    _rollout_parity(kind)


@pytest.mark.parametrize("kind", ["obb200", "moving"])
def test_rollout_parity_obstacle_gap_cost(kind):
    """Wcost[2] != 0 (simulation.cpp:91; parameters.launch:15 sets 0): the device keeps every obstacle's
    separating gap (the NEED_GAP path of the collision check) and evaluates glibc's exp, restated
    (clrrt_glibc.hpp); rollouts, rows and costS equal the oracle's bit for bit.  The reference itself reads
    the OBB normal normsY[3] that setNorms leaves unset (old_collisioncheck.cpp:74-75) in that gap; the oracle
    and the device use the edge normal, so this path is pinned to the oracle here and
    to the reference build with the stub check (tests/test_ref_tree.py, set stub_w2)."""
    def w2(p):
        p.Wcost[2] = 1.0
        return p
    _rollout_parity(kind, w2)


def _rollout_parity(kind, modify=None):
    o, pl = _pair(kind, seed=2, iters=40)
    if modify is not None:
        mode, _ = _scene(kind)
        o.set_params(modify(abi.default_params(collision_mode=mode)))
        pl.set_params(modify(clrrt.default_params(collision_mode=mode)))
    r = clrrt.Rng(11)
    smp = r.draw_samples(pl.params, 120)
    jobs = []
    for s in smp:
        ids, _ = o.sort_nodes(s.x, s.y, s.explore)
        for par in ids[:4]:
            jobs.append((par, 0, s.x, s.y))
    for par in range(o.size()):
        jobs.append((par, 1, 0.0, 0.0))
    gpu = pl.simulate_batch(jobs, rows=True)
    flips, drift = 0, []
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    for (par, gb, sx, sy), g in zip(jobs, gpu):
        c = o.simulate(par, gb, sx, sy, rows=True)
        assert g["ref_n"] == c["ref_n"]
        assert _close(g["ref_back"], c["ref_back"], 0, 0) and g["ref_vback"] == c["ref_vback"]
        if g["outcome"] != c["outcome"] or g["nrows"] != c["nrows"]:
            flips += 1
            continue
        ok = (np.array_equal(bits(g["final"]), bits(c["final"])) and g["costE"] == c["costE"]
              and g["costS"] == c["costS"] and np.array_equal(bits(g["rows"]), bits(c["rows"])))
        if not ok:
            err = np.abs(g["rows"] - c["rows"]).max(axis=1)
            drift.append((par, gb, int(np.argmax(err > 0)), float(err.max())))
    print(f"{kind}: {len(jobs)} rollouts, outcome flips {flips}, value drifts {len(drift)} {drift[:5]}")
    assert flips == 0 and not drift


@pytest.mark.parametrize("kind,strategy", [("empty", "brute"), ("obb200", "brute"), ("empty", "walk"), ("obb200", "walk"), ("moving", "walk"),
                                           ("empty", "fused"), ("obb200", "fused"), ("moving", "fused"),
                                           ("obb200", "walk_stateless"), ("obb200", "walk_split"),
                                           ("moving", "walk_split"), ("obb200", "walk_split_stateless")])
def test_nearest_node_parity(kind, strategy):
    o, pl = _pair(kind, seed=4, iters=150)
    _nn_strategy(pl, strategy)
    smp = list(clrrt.Rng(21).draw_samples(pl.params, 400))
    ids, keys = pl.sort_nodes_batch(smp)
    bad = 0
    for j, s in enumerate(smp):
        cid, ckey = o.sort_nodes(s.x, s.y, s.explore)   # std::sort, as the reference
        gid = [int(i) for i in ids[j] if i >= 0]
        if gid != cid:
            bad += 1
            print("  nn diff", j, cid, gid, ckey, list(keys[j][:len(gid)]))
            continue
        assert np.array_equal(np.asarray(keys[j][:len(cid)], np.float32).view(np.uint32),
                              np.asarray(ckey, np.float32).view(np.uint32)), j
    print(f"{kind}: {len(smp)} samples, candidate-list differences {bad}")
    assert bad == 0


def _compare_trees(o, pl, label):
    on, gn = o.nodes(), pl.nodes()
    n = min(len(on["parent"]), len(gn["parent"]))
    first_bad = None
    for i in range(n):
        same = (on["parent"][i] == gn["parent"][i] and on["goal"][i] == gn["goal"][i]
                and on["nrows"][i] == gn["nrows"][i]
                and np.array_equal(gn["state"][i].view(np.uint64), on["state"][i].view(np.uint64)))
        if not same:
            first_bad = i
            break
    print(f"{label}: oracle {len(on['parent'])} nodes, gpu {len(gn['parent'])} nodes, first divergence {first_bad}")
    return on, gn, first_bad


@pytest.mark.parametrize("kind,seed,iters,strategy", [("empty", 1, 200, "brute"), ("obb200", 3, 300, "brute"),
                                                      ("empty", 2, 300, "brute"), ("obb200", 5, 300, "brute"),
                                                      ("moving", 4, 250, "brute"), ("empty", 1, 200, "walk"),
                                                      ("obb200", 3, 300, "walk"), ("moving", 4, 250, "walk"),
                                                      ("obb200", 5, 300, "walk_stateless"),
                                                      ("obb200", 3, 300, "walk_split"),
                                                      ("empty", 1, 200, "fused"), ("obb200", 3, 300, "fused"),
                                                      ("obb200", 5, 300, "fused"), ("moving", 4, 250, "fused")])
def test_exact_mode_tree_parity(kind, seed, iters, strategy):
    """EXACT mode reproduces the reference's sequential tree (the survey's golden configurations)."""
    mode, obs = _scene(kind)
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(seed)
    o.init_tree()
    o.expand(iters)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 20,
                       max_batch=256)
    _nn_strategy(pl, strategy)
    if obs is not None:
        pl.set_obstacles(obs)
    pl.tree_init()
    rng = clrrt.Rng(seed)
    st = pl.expand(rng, n_iters=iters, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
    assert st["iterations"] == iters
    on, gn, bad = _compare_trees(o, pl, f"exact {kind} seed {seed}")
    assert bad is None and len(on["parent"]) == len(gn["parent"])
    assert np.array_equal(gn["costE"].view(np.uint32), on["costE"].view(np.uint32))
    assert np.array_equal(gn["costS"].view(np.uint32), on["costS"].view(np.uint32))
    oc, gc = o.counters(), pl.counters()
    for k in ("sim_count", "fail_collision", "fail_acclimit", "fail_iterlimit", "rollouts"):
        assert oc[k] == gc[k], (k, oc[k], gc[k])
    # trajectories (Node::tra) of every node
    for i in range(1, len(on["parent"])):
        rows = pl.rows(int(gn["row_offset"][i]), int(gn["nrows"][i]))
        assert np.array_equal(rows.view(np.uint64), np.ascontiguousarray(o.rows(i)).view(np.uint64)), i
    # the RNG state after the run equals glibc's after the same number of iterations
    ref = clrrt.Rng(seed)
    for _ in range(3 * iters):
        ref.next()
    assert bytes(ref.state) == bytes(rng.state)


@pytest.mark.parametrize("kind,batch,strategy,persistent", [("empty", 64, "brute", 1), ("obb200", 256, "brute", 1),
                                                             ("moving", 128, "brute", 1), ("obb200", 256, "brute", 0),
                                                             ("empty", 64, "walk", 1),
                                                             ("obb200", 256, "walk", 1), ("moving", 128, "walk", 1)])
def test_batch_mode_tree_parity(kind, batch, strategy, persistent):
    mode, obs = _scene(kind)
    iters = 4 * batch
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(6)
    o.init_tree()
    o.expand_batch(iters, batch, stable=True)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 21,
                       max_batch=batch)
    _nn_strategy(pl, strategy)
    pl.set_option("roll_persistent", persistent)
    if obs is not None:
        pl.set_obstacles(obs)
    pl.tree_init()
    st = pl.expand(clrrt.Rng(6), n_iters=iters, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
    assert st["iterations"] == iters and st["rounds"] == 4
    on, gn, bad = _compare_trees(o, pl, f"batch {kind} B={batch}")
    assert bad is None and len(on["parent"]) == len(gn["parent"])


@pytest.mark.parametrize("kind,batch,T,strategy,lag", [("obb200", 256, 24, "brute", 1), ("obb200", 256, 96, "walk", 1),
                                                       ("moving", 128, 40, "brute", 1), ("empty", 64, 16, "brute", 1),
                                                       ("obb200", 256, 32, "walk", 2), ("moving", 128, 8, "walk", 2)])
def test_batch_deferred_tree_parity(kind, batch, T, strategy, lag):
    """BATCH rounds with deferred samples (option defer_steps T): the rollout chains run at most T steps per
    launch, suspended chains resume in the next launch, and a sample commits at the first commit after which
    every rollout its result depends on has ended -- ceil(chain / T) - 1 rounds after its own (the oracle's
    orc_expand_batch_defer).  The tree equals the oracle's node for node, bit for bit (rows and counters too),
    with the lag-1 and lag-2 pipelines."""
    mode, obs = _scene(kind)
    iters = 6 * batch
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(6)
    o.init_tree()
    ndef = o.expand_batch(iters, batch, stable=True, defer_steps=T)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 21,
                       max_batch=batch)
    _nn_strategy(pl, strategy)
    pl.set_option("defer_steps", T)
    pl.set_option("nn_lag", lag)
    if obs is not None:
        pl.set_obstacles(obs)
    pl.tree_init()
    st = pl.expand(clrrt.Rng(6), n_iters=iters, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
    assert st["iterations"] == iters and st["rounds"] == 6
    print(f"defer T={T}: {ndef} of {iters} samples deferred by the oracle")
    assert ndef > 0
    on, gn, bad = _compare_trees(o, pl, f"batch deferred {kind} B={batch} T={T} lag {lag}")
    assert bad is None and len(on["parent"]) == len(gn["parent"])
    assert np.array_equal(gn["costS"].view(np.uint32), on["costS"].view(np.uint32))
    oc, gc = o.counters(), pl.counters()
    for k in ("sim_count", "fail_collision", "fail_acclimit", "fail_iterlimit", "rollouts"):
        assert oc[k] == gc[k], (k, oc[k], gc[k])
    for i in range(1, len(on["parent"])):
        rows = pl.rows(int(gn["row_offset"][i]), int(gn["nrows"][i]))
        assert np.array_equal(rows.view(np.uint64), np.ascontiguousarray(o.rows(i)).view(np.uint64)), i
    assert pl.debug_counters()[61] == 0


def test_lockstep_iteration_parity():
    """Every iteration of a sequential oracle run, evaluated by the GPU on the oracle's own tree."""
    mode, obs = _scene("obb200")
    q = abi.default_params(collision_mode=mode)
    o = Oracle(q, obs)
    Oracle.srand(8)
    o.init_tree()
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 14, max_rows=1 << 20,
                       max_batch=4)
    pl.set_obstacles(obs)
    import torch
    out = torch.empty((2, 160), dtype=torch.uint8, device="cuda")
    mism = 0
    for it in range(120):
        xy, ex = o.draw_samples(1)
        pl.tree_load(o.nodes_raw())
        smp = (abi.Sample * 1)()
        smp[0].x, smp[0].y, smp[0].explore = xy[0][0], xy[0][1], int(ex[0])
        n = pl.round_eval(smp, out.data_ptr())
        ref = o.eval_iteration(xy[0][0], xy[0][1], ex[0], stable=True)
        got = out[:n].cpu().numpy().tobytes()
        g = clrrt.nodes_to_numpy((abi.Node * n).from_buffer_copy(got)) if n else None
        if n != len(ref):
            mism += 1
        elif n:
            r = clrrt.nodes_to_numpy((abi.Node * n)(*ref))
            if not (np.array_equal(g["nrows"], r["nrows"]) and np.array_equal(g["state"].view(np.uint64),
                                                                               r["state"].view(np.uint64))):
                mism += 1
        # advance the oracle with the same iteration (rand() already consumed by draw_samples)
        _append_ref(o, ref, o.size())
    print(f"lockstep: 120 iterations, mismatches {mism}")
    assert mism == 0


def _append_ref(o, ref_nodes, base):
    """Append evaluated nodes to the oracle tree through its loader (headers are all expansion reads)."""
    if not ref_nodes:
        return
    cur = list(o.nodes_raw())
    for k, nd in enumerate(ref_nodes):
        if nd.parent == -2:
            nd.parent = base + k - 1
        cur.append(nd)
    arr = (abi.Node * len(cur))(*cur)
    o.load_tree(arr)


def _bitwise_report(gn, on, label):
    """Count nodes whose FP64 state differs from the oracle's in any bit (expected: none)."""
    diff = int(np.sum(np.any(gn["state"].view(np.uint64) != on["state"].view(np.uint64), axis=1)))
    print(f"{label}: nodes with any state bit different: {diff}")
    return diff


@pytest.mark.parametrize("kind,seed,iters", [("obb200", 3, 300), ("moving", 4, 250)])
def test_exact_mode_bitwise(kind, seed, iters):
    """The EXACT-mode tree is bit-identical to the oracle's: node states, float costs, rows."""
    mode, obs = _scene(kind)
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(seed)
    o.init_tree()
    o.expand(iters)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 20,
                       max_batch=256)
    pl.set_obstacles(obs)
    pl.tree_init()
    pl.expand(clrrt.Rng(seed), n_iters=iters, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
    on, gn = o.nodes(), pl.nodes()
    assert len(on["parent"]) == len(gn["parent"])
    assert _bitwise_report(gn, on, f"{kind} seed {seed}") == 0
    assert np.array_equal(gn["costE"].view(np.uint32), on["costE"].view(np.uint32))
    assert np.array_equal(gn["costS"].view(np.uint32), on["costS"].view(np.uint32))
    for i in range(1, len(on["parent"])):
        rows = pl.rows(int(gn["row_offset"][i]), int(gn["nrows"][i]))
        assert np.array_equal(rows.view(np.uint64), np.ascontiguousarray(o.rows(i)).view(np.uint64)), i


def test_walk_matches_brute_force_large_tree():
    """Full-size property: on a BATCH-grown tree of ~100k nodes the walk searches return exactly the
    brute-force candidate lists (ids and keys) for every sample of a 16384-sample batch."""
    mode, obs = _scene("obb200")
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 20, max_rows=1 << 26,
                       max_batch=16384)
    pl.set_obstacles(obs)
    pl.tree_init()
    pl.expand(clrrt.Rng(9), n_iters=16384 * 8, mode=clrrt.CLRRT_MODE_BATCH, batch=16384)
    n_nodes = pl.size()[0]
    assert n_nodes > 20000
    smp = list(clrrt.Rng(33).draw_samples(pl.params, 16384))
    _nn_strategy(pl, "brute")
    ids_b, keys_b = pl.sort_nodes_batch(smp, exact=False)
    for strategy in ("walk", "walk_stateless", "walk_coded", "walk_split_coded", "walk_persistent",
                     "walk_coded_persistent", "walk_split_persistent"):
        _nn_strategy(pl, strategy)
        ids_g, keys_g = pl.sort_nodes_batch(smp, exact=False)
        print(f"tree {n_nodes} nodes; {strategy} lists equal: {np.array_equal(ids_b, ids_g)}")
        assert np.array_equal(ids_b, ids_g)
        assert np.array_equal(keys_b.view(np.uint32)[ids_b >= 0], keys_g.view(np.uint32)[ids_g >= 0])
    # and against the oracle's std::sort on a subset
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    o.load_tree(pl.nodes_raw())
    for j in range(0, 16384, 1024):
        s = smp[j]
        cid, _ = o.sort_nodes(s.x, s.y, s.explore, stable=True)
        assert [int(i) for i in ids_g[j] if i >= 0] == cid, j


@pytest.mark.gpu
def test_pipelined_batch_rounds_identical():
    """Full-size property: BATCH rounds with the walk search of the round after next (nn_lag 2, the default for
    long queries, with or without its stream priorities, or of the
    next round: nn_lag 1) overlapped with the current
    round's rollouts (+ the merge of the appended nodes, launch_nn_delta) grow exactly the tree of
    plain rounds (every node record and trajectory row).  So do the scheduling and search options: the
    rollout queue order (roll_priority), the persistent grid width (roll_blocks), the per-lane collision
    checks instead of the wave-cooperative ones (roll_coop), the single-buffered
    walk index (nn_walk_double) and the walk without overflow split (budget 0) or with every sample
    split (budget 1); and the trajectory rows stored by every speculative rollout (rows_deferred 0) instead of
    replayed for the accepted ones only (the default: each replay must run exactly its node's row count)."""
    mode, obs = _scene("obb200")
    trees = []
    variants = [dict(nn_pipeline=0), dict(nn_pipeline=1), dict(nn_lag=1), dict(nn_lag=2),
                dict(nn_lag=2, stream_prio=0), dict(roll_priority=0, roll_blocks=512),
                dict(roll_coop=0), dict(rows_deferred=0),
                dict(nn_walk_double=0), dict(nn_walk_budget_tiles=0, nn_walk_budget_keys=0),
                dict(nn_walk_budget_tiles=1, nn_walk_budget_keys=1, nn_walk_chunks=5),
                # a scheduling option (32 job lanes per wave) and the large-tree walk format
                dict(roll_lanes=32),
                dict(nn_walk_stateless=1, nn_walk_half_max=0), dict(nn_walk_waves=0), dict(nn_walk_waves=512)]
    for opts in variants:
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 20, max_rows=1 << 26,
                           max_batch=16384)
        for k, v in opts.items():
            pl.set_option(k, v)
        pl.set_obstacles(obs)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(12), n_iters=16384 * 6, mode=clrrt.CLRRT_MODE_BATCH, batch=16384)
        assert st["rounds"] == 6
        n, nr = pl.size()
        trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), n))
        d = pl.debug_counters()
        assert d[61] == 0, f"{d[61]} replays ran a different row count ({opts})"
        assert (d[60] > 0) == (opts.get("rows_deferred", 1) != 0), (d[60], opts)
        pl.close()
    print(f"pipelined rounds: {trees[1][2]} nodes")
    assert trees[0][2] > 20000
    for t in trees[1:]:
        assert trees[0][0] == t[0] and trees[0][1] == t[1]


RETIRED_OPTIONS = ("cu_split", "walk_cu_reserve", "side_priority", "nn_walk_lpt", "nn_walk_lds_floor",
                   "nn_delta_early", "nn_lane_order")


@pytest.mark.gpu
def test_retired_options_rejected_without_state():
    """The scheduling options retired after their A/B measurements ("Options retired") are
    unknown keys: clrrt_set_option returns CLRRT_EINVAL (-1) for each, and a planner that was asked for all seven
    grows, byte for byte, the tree and rows of a fresh planner -- a rejected key leaves no state behind."""
    mode, obs = _scene("obb200")
    trees = []
    for ask in (True, False):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 12, max_rows=1 << 22,
                           max_batch=64)
        try:
            if ask:
                for key in RETIRED_OPTIONS:
                    with pytest.raises(clrrt.ClrrtError, match=r"-> -1: unknown option or value: " + key):
                        pl.set_option(key, 1)
            pl.set_option("nn_walk_min", 64)
            pl.set_option("nn_lag", 2)
            pl.set_obstacles(obs)
            pl.tree_init()
            st = pl.expand(clrrt.Rng(12), n_iters=64 * 3, mode=clrrt.CLRRT_MODE_BATCH, batch=64)
            assert st["rounds"] == 3
            n, nr = pl.size()
            trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), n))
        finally:
            pl.close()
    assert trees[0][2] > 1
    assert trees[0] == trees[1]


@pytest.mark.gpu
def test_exact_min_width_identical():
    """EXACT trees do not depend on the speculation width (option exact_min_width): the committed prefix of
    every round is the reference's sequential order, whatever the number of samples speculated."""
    mode, obs = _scene("obb200")
    trees = []
    for width in (8, 64, 1):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 22,
                           max_batch=256)
        pl.set_option("exact_min_width", width)
        pl.set_obstacles(obs)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(21), n_iters=300, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
        assert st["iterations"] == 300
        n, nr = pl.size()
        trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes()))
        pl.close()
    assert trees[0] == trees[1] == trees[2]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed,iters", [("obb200", 3, 400), ("moving", 4, 300), ("empty", 2, 300)])
def test_exact_fixups_identical(kind, seed, iters):
    """EXACT rounds with fix-ups (option exact_fixup, the default: a conflicting sample stands when the new nodes
    that enter its list before its result all fail their rollouts for it) grow the tree of rounds without them
    and of the oracle's sequential expandTree, node for node, rows and counters too -- and they resolve conflicts."""
    mode, obs = _scene(kind)
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(seed)
    o.init_tree()
    o.expand(iters)
    trees = []
    for fix in (1, 0):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 16, max_rows=1 << 22,
                           max_batch=256)
        pl.set_option("exact_fixup", fix)
        if obs is not None:
            pl.set_obstacles(obs)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(seed), n_iters=iters, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
        assert st["iterations"] == iters
        n, nr = pl.size()
        trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), pl.counters(), st["rounds"], pl.exact_stats()))
        if fix:
            on, gn, bad = _compare_trees(o, pl, f"exact fix-ups {kind} seed {seed}")
            assert bad is None and len(on["parent"]) == len(gn["parent"])
            oc = o.counters()
            for k in ("sim_count", "fail_collision", "fail_acclimit", "fail_iterlimit", "rollouts"):
                assert oc[k] == trees[-1][2][k], (k, oc[k], trees[-1][2][k])
        pl.close()
    print(f"{kind}: rounds with fix-ups {trees[0][3]} vs {trees[1][3]} without; stats {trees[0][4]}")
    assert trees[0][0] == trees[1][0] and trees[0][1] == trees[1][1] and trees[0][2] == trees[1][2]
    if kind != "empty":
        assert trees[0][4]["resolved"] > 0 and trees[0][3] < trees[1][3]


@pytest.mark.gpu
def test_deferred_batch_rounds_identical():
    """Full-size property of the deferred-sample rounds (defer_steps 128, as bench.py runs cfg3): the pipelines (none, lag 1, lag 2) and
    the scheduling options (grid width, queue order, per-lane collision checks) grow exactly the same tree --
    which samples are deferred, and by how many rounds, depends on their rollouts' step counts only -- and
    a sample is deferred in every variant; rows of every node replay exactly."""
    mode, obs = _scene("obb200")
    trees = []
    variants = [dict(nn_pipeline=0), dict(nn_lag=1), dict(nn_lag=2), dict(nn_lag=2, roll_priority=0, roll_blocks=512),
                dict(nn_lag=1, roll_coop=0, roll_blocks=64)]
    for opts in variants:
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 20, max_rows=1 << 26,
                           max_batch=16384)
        pl.set_option("defer_steps", 128)  # the cfg3 bench setting
        for k, v in opts.items():
            pl.set_option(k, v)
        pl.set_obstacles(obs)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(12), n_iters=16384 * 6, mode=clrrt.CLRRT_MODE_BATCH, batch=16384)
        assert st["rounds"] == 6 and st["deferred"] > 0, st
        n, nr = pl.size()
        trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), n, st["deferred"]))
        assert pl.debug_counters()[61] == 0
        pl.close()
    print(f"deferred rounds: {trees[0][2]} nodes, {trees[0][3]} samples deferred")
    assert trees[0][2] > 20000
    for t in trees[1:]:
        assert trees[0][0] == t[0] and trees[0][1] == t[1] and trees[0][3] == t[3]


@pytest.mark.gpu
def test_round_prefetch_identical():
    """The multi-GPU round API with clrrt_round_prefetch (the next shard's search beside this round's
    rollouts, merged with the committed nodes) grows exactly the tree of plain round_eval/commit."""
    import torch
    mode, obs = _scene("obb200")
    B, rounds = 16384, 5
    trees = []
    for pre in (False, True):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 20, max_rows=1 << 26,
                           max_batch=B)
        pl.set_obstacles(obs)
        pl.tree_init()
        out = torch.empty((2 * B, 160), dtype=torch.uint8, device="cuda")
        rng = clrrt.Rng(14)
        nxt = rng.draw_samples(pl.params, B)
        for _ in range(rounds):
            cur, nxt = nxt, rng.draw_samples(pl.params, B)
            if pre:
                pl.round_prefetch(nxt)
            n = pl.round_eval(cur, out.data_ptr())
            pl.round_commit(out.data_ptr(), n, 0, n)
        n_nodes, nr = pl.size()
        trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), n_nodes))
        assert pl.debug_counters()[61] == 0
        pl.close()
    print(f"round prefetch: {trees[1][2]} nodes")
    assert trees[0][2] > 20000
    assert trees[0][0] == trees[1][0] and trees[0][1] == trees[1][1]


@pytest.mark.parametrize("chunks", [1, 32, 64])
def test_walk_overflow_matches_brute(chunks):
    """More overflowing samples than overflow records (512): the first 512 go through the split waves
    and the merge, the rest finish their own walk; every list equals the brute force's bit for bit."""
    o, pl = _pair("obb200", seed=6, iters=300)
    smp = list(clrrt.Rng(23).draw_samples(pl.params, 2000))
    _nn_strategy(pl, "brute")
    ib, kb = pl.sort_nodes_batch(smp)
    _nn_strategy(pl, "walk_split")
    pl.set_option("nn_walk_chunks", chunks)
    pl.set_option("nn_walk_max_over", 512)
    pl.reset_counters()
    iw, kw = pl.sort_nodes_batch(smp)
    records = pl.debug_counters()[32]
    print(f"{o.size()} nodes, {len(smp)} samples, overflow records {records}")
    assert records == 512
    assert np.array_equal(ib, iw)
    assert np.array_equal(np.asarray(kb, np.float32).view(np.uint32), np.asarray(kw, np.float32).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("mode_name", ["EXACT", "BATCH"])
def test_budget_loop_termination_and_draws(mode_name):
    """SURVEY §8(a) a13, the Timer(200) loop of planMotion (motionplanner.cpp:39-43) as clrrt_expand with a
    wall-clock budget: it stops once 200 ms have elapsed (checked between rounds), consumes exactly three
    rand() draws per counted iteration (the returned RNG state equals a fresh stream advanced 3 x
    iterations), and its tree equals the fixed-count expansion of the same number of iterations."""
    mode, obs = _scene("obb200")
    m = clrrt.CLRRT_MODE_EXACT if mode_name == "EXACT" else clrrt.CLRRT_MODE_BATCH
    batch = 256 if mode_name == "EXACT" else 4096
    trees, its = [], None
    for fixed in (False, True):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 20, max_rows=1 << 26,
                           max_batch=batch)
        pl.set_obstacles(obs)
        pl.tree_init()
        rng = clrrt.Rng(9)
        if not fixed:
            st = pl.expand(rng, n_iters=0, budget_ms=200.0, mode=m, batch=batch)
            its = st["iterations"]
            assert its > 0 and st["elapsed_ms"] >= 200.0, st
            assert st["elapsed_ms"] < 200.0 + 5000.0, st
            if m == clrrt.CLRRT_MODE_BATCH:
                assert its % batch == 0, st
            ref = clrrt.Rng(9)
            for _ in range(3 * its):
                ref.next()
            assert bytes(rng.state) == bytes(ref.state)
        else:
            st = pl.expand(rng, n_iters=its, mode=m, batch=batch)
            assert st["iterations"] == its
        n, nr = pl.size()
        trees.append((bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes()))
        pl.close()
    print(mode_name, "budget 200 ms:", its, "iterations")
    assert trees[0] == trees[1]
