"""Deferred rounds at full-horizon chains, and the BATCH paths under non-default queries -- GPU against the oracle.

The cases are tests/query_cases.py's; tests/test_query_space_oracle.py shows on the oracle alone that each one
reaches what it is listed for.  Tolerance: none (tests/test_gpu_parity.py): node headers, costE / costS bits,
every trajectory row and the five counters equal the oracle's.

1. test_long_chains_*: chains of up to 2 n_steps_max steps through the deferral rings (ensure_defer's
   R = ceil(2 n_steps_max / T) + 2 round slots, d.slot = round % R), with more rounds than R, so slots are reused
   while samples of up to ceil(2 n_steps_max / T) earlier rounds are still in flight.
2. test_query_space_batch: each query-space case at (T 0, brute), (T 32, walk, lag 2), (T 32, walk_split, lag 1).
3. test_units_under_case_parameters: candidate lists and single rollouts on the oracle's tree under the same
   parameters, so that a tree mismatch above points at a kernel.
4. test_one_context_changing_queries: one context through queries that change sim_dt, T and the paths that store
   rows in slots (the regrow branches of ensure_defer, clrrt_set_params and ensure_slots).
5. test_exact_under_case_parameters: EXACT mode under two of the cases' parameters.
"""
import numpy as np
import pytest

import clrrt
import query_cases as qc
from test_gpu_parity import _nn_strategy

pytestmark = pytest.mark.gpu


def _planner(p, obs, root, batch, opts=(), strategy=None, max_nodes=1 << 14, max_rows=1 << 22):
    pl = clrrt.Planner(p, max_nodes=max_nodes, max_rows=max_rows, max_batch=batch)
    if strategy is not None:
        _nn_strategy(pl, strategy)
    for k, v in dict(opts).items():
        pl.set_option(k, v)
    if obs is not None:
        pl.set_obstacles(obs)
    pl.tree_init(root)
    return pl


def _assert_clean(pl, label):
    """No replay ran another row count than its node's (work counter 61), no rollout wave hit the watchdog (56-59)."""
    d = pl.debug_counters()
    assert d[61] == 0, (label, d[61])
    assert d[56:60] == [0, 0, 0, 0], (label, d[56:60])
    return d


def _batch_against_oracle(name, T, opts, strategy, label, rows=True):
    """The case's BATCH expansion on the device (options opts + defer_steps T) against the oracle's tree."""
    c = qc.case(name)
    B, rounds = (c["B"], c["rounds"]) if name in qc.LONG else (qc.QUERY_B, qc.QUERY_ROUNDS)
    o, ndef = qc.grown(name, T)
    p, root, obs = qc.make(name)
    pl = _planner(p, obs, root, B, dict(opts, defer_steps=T), strategy)
    try:
        st = pl.expand(clrrt.Rng(qc.SEED), n_iters=B * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
        print(f"{label}: {st}")
        assert st["iterations"] == B * rounds and st["rounds"] == rounds and st["capacity_stop"] == 0, st
        qc.assert_tree_equal(o, pl, label, rows=rows)
        assert st["deferred"] == ndef, (label, st["deferred"], ndef)
        return _assert_clean(pl, label)
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------- 1. long chains
@pytest.mark.parametrize("lag", [1, 2])
@pytest.mark.parametrize("name", list(qc.LONG))
def test_long_chains_through_the_deferred_pipeline(name, lag):
    """More rounds than ring slots, chains past n_steps_max in flight (up to 24 launches for one sample), the
    pipelined walk search of the next round (lag 1) or the round after next (lag 2) beside the rollouts."""
    T = qc.LONG[name]["T"]
    _batch_against_oracle(name, T, dict(nn_lag=lag, nn_walk_min=0), None, f"{name} T {T} lag {lag}")


@pytest.mark.parametrize("priority,verify", [(0, 0), (1, 0), (1, 1)])
def test_long_chains_queue_order(priority, verify):
    """slow_T128 under the plain queue order, the order by length class (k_roll_flag scales its classes by the cap T,
    or by n_steps_max) and the order checked on the device: positions checked > 0, wrong 0 (tests/test_roll_order.py).
    roll_blocks 2: the queue is longer than the grid's lanes, so it is served by class."""
    d = _batch_against_oracle("slow_T128", 128, dict(roll_priority=priority, roll_order_verify=verify, roll_blocks=2),
                              None, f"slow_T128 roll_priority {priority} verify {verify}")
    if verify:
        print(f"order: positions checked {d[6]}, wrong {d[7]}")
        assert d[6] > 0
        assert d[7] == 0


def test_long_chains_rows_in_slots():
    """slow_dt10_T64's query without deferral on the non-persistent rollout kernel: every speculative rollout stores
    its rows in its job's slot (201 rows per slot, sized by n_steps_max), accepted ones are copied to the arena."""
    _batch_against_oracle("slow_dt10_T64", 0, dict(roll_persistent=0), None, "slow_dt10_T64 T 0 roll_persistent 0")


# ---------------------------------------------------------------------------------------------- 2. query space
SETTINGS = [(0, "brute", dict()), (32, "walk", dict(nn_lag=2)), (32, "walk_split", dict(nn_lag=1))]


@pytest.mark.parametrize("name", list(qc.QUERY))
def test_query_space_batch(name):
    for T, strategy, opts in SETTINGS:
        _batch_against_oracle(name, T, opts, strategy, f"{name} T {T} {strategy} {opts}")


# ---------------------------------------------------------------------------------------------- 3. units
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["fast", "goal_far", "dt02", "bend_w2", "slow_T128"])
def test_units_under_case_parameters(name):
    """The oracle's tree after 2 plain rounds, loaded into the device: sort_nodes_batch of 400 fresh samples against
    the oracle's std::sort lists (ids and float key bits; brute force and the walk), and simulate_batch of the
    first 4 candidates per sample + one goal-biased job per node against the oracle's Simulation (outcome, row
    count, state bits, costs, rows)."""
    p, root, obs = qc.make(name)
    o, _ = qc.grown(name, 0, rounds=2)
    assert o.size() >= 40, o.size()
    pl = clrrt.Planner(p, max_nodes=1 << 14, max_rows=1 << 20, max_batch=512)
    try:
        if obs is not None:
            pl.set_obstacles(obs)
        pl.tree_load(o.nodes_raw())
        smp = list(clrrt.Rng(21).draw_samples(p, 400))
        lists = [o.sort_nodes(s.x, s.y, s.explore) for s in smp]   # std::sort, as the reference
        assert sum(len(cid) for cid, _ in lists) > 400
        for strategy in ("brute", "walk"):
            _nn_strategy(pl, strategy)
            ids, keys = pl.sort_nodes_batch(smp)
            bad = 0
            for j, (cid, ckey) in enumerate(lists):
                gid = [int(i) for i in ids[j] if i >= 0]
                if gid != cid:
                    bad += 1
                    print("  nn diff", strategy, j, cid, gid, ckey, list(keys[j][:len(gid)]))
                    continue
                assert np.array_equal(np.asarray(keys[j][:len(cid)], np.float32).view(np.uint32),
                                      np.asarray(ckey, np.float32).view(np.uint32)), (strategy, j)
            print(f"{name} {strategy}: {o.size()} nodes, {len(smp)} samples, candidate-list differences {bad}")
            assert bad == 0
        jobs = [(par, 0, s.x, s.y) for s, (cid, _) in zip(smp, lists) for par in cid[:4]]
        jobs += [(par, 1, 0.0, 0.0) for par in range(o.size())]
        cap = qc.n_steps_max(p) + 1
        flips, drift, outcomes = 0, [], {}
        for j0 in range(0, len(jobs), 512):
            chunk = jobs[j0:j0 + 512]
            for (par, gb, sx, sy), g in zip(chunk, pl.simulate_batch(chunk, rows=True)):
                c = o.simulate(par, gb, sx, sy, rows=True, rows_cap=cap)
                outcomes[c["outcome"]] = outcomes.get(c["outcome"], 0) + 1
                assert g["ref_n"] == c["ref_n"]
                assert np.array_equal(_bits(g["ref_back"]), _bits(c["ref_back"])) and g["ref_vback"] == c["ref_vback"]
                if g["outcome"] != c["outcome"] or g["nrows"] != c["nrows"]:
                    flips += 1
                    continue
                ok = (np.array_equal(_bits(g["final"]), _bits(c["final"])) and g["costE"] == c["costE"]
                      and g["costS"] == c["costS"] and np.array_equal(_bits(g["rows"]), _bits(c["rows"])))
                if not ok:
                    drift.append((par, gb, sx, sy))
        print(f"{name}: {len(jobs)} rollouts {outcomes}, outcome flips {flips}, value drifts {len(drift)} {drift[:5]}")
        assert flips == 0 and not drift
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------- 4. one context
# (case, defer_steps T, further options); the two queries after the issue's five store rows in slots
# (rows_deferred 0): the first allocates them at 201 rows (ensure_slots), the second's clrrt_set_params regrows
# them to 1001
SEQUENCE = [("default", 128, {}), ("dt02", 128, {}), ("default", 16, {}), ("slow_dt10_T64", 64, {}), ("fast", 0, {}),
            ("dt10", 0, dict(rows_deferred=0)), ("dt02", 0, dict(rows_deferred=0))]


def test_one_context_changing_queries():
    """A host changes the query on every call.  One context, max_batch 128: each query is set_params,
    set_obstacles, tree_init(root) and 6 rounds, and its tree equals a fresh oracle's.  The rings grow when sim_dt
    shrinks (default -> dt02: R 10 -> 18) and when T does (T 128 -> 16: R 65), and a later query with fewer slots
    in use (slow_dt10, R 9) runs in the larger ring."""
    B, rounds = 128, 6
    p0, root0, obs0 = qc.make("default")
    pl = clrrt.Planner(p0, max_nodes=1 << 14, max_rows=1 << 22, max_batch=B)
    try:
        for name, T, opts in SEQUENCE:
            p, root, obs = qc.make(name)
            o, ndef = qc.grown(name, T, B=B, rounds=rounds)
            pl.set_option("rows_deferred", 1)
            for k, v in dict(opts, defer_steps=T).items():
                pl.set_option(k, v)
            pl.set_params(p)
            pl.set_obstacles(obs if obs is not None else np.zeros((0, 7)))
            pl.tree_init(root)
            pl.reset_counters()
            st = pl.expand(clrrt.Rng(qc.SEED), n_iters=B * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
            label = f"one context: {name} T {T} {opts}"
            print(f"{label}: {st}")
            assert st["iterations"] == B * rounds and st["rounds"] == rounds and st["capacity_stop"] == 0, st
            assert o.size() >= 50, (label, o.size())
            qc.assert_tree_equal(o, pl, label)
            assert st["deferred"] == ndef and (ndef > 0) == (T > 0), (label, st["deferred"], ndef)
            _assert_clean(pl, label)
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------- 5. EXACT
@pytest.mark.parametrize("name,scene", [("slow_T128", "S"), ("fast", "M")])
def test_exact_under_case_parameters(name, scene):
    iters = 300
    p, root, obs = qc.make(name, scene)
    o = qc.fresh_oracle(name, scene)
    o.expand(iters)
    pl = _planner(p, obs, root, 256, max_rows=1 << 21)
    try:
        rng = clrrt.Rng(qc.SEED)
        st = pl.expand(rng, n_iters=iters, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
        assert st["iterations"] == iters
        assert o.size() >= 50, o.size()
        qc.assert_tree_equal(o, pl, f"exact {name} scene {scene}")
        ref = clrrt.Rng(qc.SEED)   # three rand() draws per iteration
        for _ in range(3 * iters):
            ref.next()
        assert bytes(ref.state) == bytes(rng.state)
        _assert_clean(pl, f"exact {name}")
    finally:
        pl.close()
