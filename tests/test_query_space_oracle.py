"""The query-space cases (tests/query_cases.py) exercise what they are listed for -- CPU, the oracle alone.

Conditions on the inputs of tests/test_query_space.py, not on the device: a long-chain case has to run more
rounds than the deferral ring has slots, with chains past n_steps_max in flight; a query-space case has to grow a
tree worth comparing and reach the outcome its parameters are there for.  Each threshold is set well below what
the oracle gave when the case was chosen (the "oracle" entry of the tables); a case that stops qualifying is to
be replaced, not the threshold.
"""
import math

import numpy as np
import pytest

import query_cases as qc

MIN_LAUNCHES = {"slow_dt10_T16": 20, "slow_T128": 5, "slow_goal_T128_stub": 5}


@pytest.mark.parametrize("name", list(qc.LONG))
def test_long_chain_case_wraps_the_ring(name):
    c = qc.LONG[name]
    p, _, _ = qc.make(name)
    n, R = qc.n_steps_max(p), qc.ring_slots(p, c["T"])
    o, ndef = qc.grown(name)
    on, cnt = o.nodes(), o.counters()
    ch = qc.accepted_chains(on)
    over = int((ch > n).sum())
    launches = math.ceil(int(ch.max()) / c["T"])
    print(f"{name}: n_steps_max {n}, R {R}, rounds {c['rounds']}; {o.size()} nodes, {int((on['goal'] == 1).sum())} goal, "
          f"deferred {ndef}, iterlimit {cnt['fail_iterlimit']}, accepted chains > {n}: {over}, longest {int(ch.max())} "
          f"({launches} launches)")
    assert c["rounds"] > R
    assert ndef > 0
    assert cnt["fail_iterlimit"] >= 100
    assert over >= 5
    assert int(ch.max()) <= 2 * n  # the bound the ring is sized for
    if name in MIN_LAUNCHES:
        assert launches >= MIN_LAUNCHES[name]


@pytest.mark.parametrize("name", list(qc.QUERY))
def test_query_case_reaches_its_target(name):
    for T in qc.QUERY_TS:
        o, ndef = qc.grown(name, T)
        on, cnt = o.nodes(), o.counters()
        goal = int((on["goal"] == 1).sum())
        print(f"{name} T {T}: {o.size()} nodes, {goal} goal, deferred {ndef}, {cnt}, rows to {int(on['nrows'].max())}")
        assert o.size() >= 100
        if T > 0:
            assert (ndef == 0) if name in qc.NO_DEFERRAL else (ndef > 0)
        else:
            assert ndef == 0
        if name in ("fast", "fast_v20"):
            assert cnt["fail_acclimit"] >= 500
        if name in ("goal_near", "fast_stub"):
            assert goal >= 50
        if name == "goal_right":
            assert cnt["fail_iterlimit"] > 0


def test_query_case_parameters():
    """The derived quantities the cases are there to move."""
    ref_res = {n: qc.make(n)[0].ref_res for n in qc.QUERY}
    assert ref_res["fast"] == 12.0 * 0.02 and ref_res["fast_v20"] == 20.0 * 0.02  # feas_len 0.504, 0.84
    assert all(r == 0.2 for n, r in ref_res.items() if not n.startswith("fast"))
    assert qc.n_steps_max(qc.make("dt02")[0]) == 1000 and qc.n_steps_max(qc.make("dt10")[0]) == 200
    assert qc.n_steps_max(qc.make("default")[0]) == 500
    p = qc.make("bend_w2")[0]
    assert (p.bend, p.lane_shift0, tuple(p.Cxy), p.Wcost[2]) == (1, 0.5, (0.0, 0.05, -1.0), 1.0)
    assert qc.make("sort1")[0].sort_limit == 1 and qc.make("nopred")[0].obs_use_pred == 0
    assert [qc.ring_slots(qc.make(n)[0], c["T"]) for n, c in qc.LONG.items()] == [27, 9, 27, 10, 10]


@pytest.mark.parametrize("name", ["slow_dt10_T16_stub", "slow_dt10_T64"])
def test_threaded_expansion_equals_serial(name):
    """expand_batch(threads=16), which the GPU tests' trees are grown with, equals threads=0."""
    ot, dt = qc.grown(name)
    os_, ds = qc.grown(name, threads=0)
    assert dt == ds and ot.size() == os_.size()
    assert bytes(ot.nodes_raw()) == bytes(os_.nodes_raw())
    assert ot.counters() == os_.counters()
    for i in range(1, ot.size()):
        assert np.array_equal(ot.rows(i).view(np.uint64), os_.rows(i).view(np.uint64)), i
