"""EXACT rounds, iteration by iteration: the decision logic that makes speculative rounds equal the reference's
sequential expandTree -- k_conflict / k_conflict_fix (clrrt_kernels.hip), exact_fixups (clrrt_capi.hip) and the
change of list kernels at 12000 nodes -- against the oracle stepped one iteration at a time.

Tolerance: none.  Tree (every header field both sides carry), the rows of every appended node, the counters' totals
and every field of every clrrt_iteration record must equal the oracle's, bit for bit.  The per-iteration records are
the interface a caller of the adapter's expandTree sees; totals alone let a wrong fix_adj sign cancel against an
opposite error elsewhere.  Cases, references and comparisons: tests/exact_cases.py.
"""
import numpy as np
import pytest

import clrrt
from clrrt import abi
import exact_cases as X
from oracle_binding import Oracle

SCENES = [("obb200", 3, 400), ("moving", 4, 300), ("empty", 2, 300)]  # those of test_exact_fixups_identical
CAP = 48


def _fresh(kind, seed, iters, batch=256):
    return ("fresh", kind, seed, iters, batch, 0, 0)


# --------------------------------------------------------------------------------------------- 1. host checks
@pytest.mark.parametrize("kind,seed,iters", SCENES)
def test_oracle_single_steps_equal_one_call(kind, seed, iters):
    """What the per-iteration reference rests on: expand(1) called n times after srand(seed) leaves the tree bytes and
    counters of one expand(n).  (No GPU.)"""
    mode, obs = X.scene(kind)
    o = Oracle(abi.default_params(collision_mode=mode), obs)
    Oracle.srand(seed)
    o.init_tree()
    o.expand(iters)
    step = X.make_oracle(_fresh(kind, seed, iters))
    rec = X.oracle_steps(step, iters)
    assert bytes(o.nodes_raw()) == bytes(step.nodes_raw())
    assert o.counters() == step.counters()
    for i in range(o.size()):
        assert np.array_equal(o.rows(i).view(np.uint64), step.rows(i).view(np.uint64)), i
    # the deltas add up to the totals, and an iteration appends 0, 1 or 2 nodes
    assert set(np.unique(rec[:, 0])) <= {0, 1, 2} and rec[:, 0].sum() == o.size() - 1
    assert rec[:, 1:].sum(axis=0).tolist() == [o.counters()[k] for k in X.COUNTERS]
    # the cached reference is this run
    assert np.array_equal(X.reference(_fresh(kind, seed, iters))["records"], rec)


def test_cap_is_reached_by_the_chosen_seeds():
    """The coverage condition of exact_fixup_cap 48, selected on the CPU: in every scene's run some iteration tries,
    before its result, a node appended by one of the two iterations before it whose rollout for the sample (the
    oracle's simulate of the same parent and sample) runs more than 48 steps.  In EXACT rounds that is a fix-up
    rollout which the cap stops undecided.  (No GPU; test_cap_changes_rounds_not_results shows the engine meets it.)"""
    for kind, seed, iters in SCENES:
        hits = X.cap_reaching_iterations(_fresh(kind, seed, iters), CAP)
        print(kind, seed, "iterations with a fix-up rollout past the cap:", hits)
        assert hits, (kind, seed)


# --------------------------------------------------------------------------------------------- 1. engine runs
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, CAP])
@pytest.mark.parametrize("width", [1, 8, 64])
@pytest.mark.parametrize("fix", [1, 0])
@pytest.mark.parametrize("kind,seed,iters", SCENES)
def test_iteration_records_equal_sequential_oracle(kind, seed, iters, fix, width, cap):
    """Whatever the fix-up setting, the speculation width and the fix-up rollouts' step cap: each committed iteration
    appends the nodes and adds the counters of the oracle's iteration of the same number."""
    case = _fresh(kind, seed, iters)
    pl, st, rec = X.run_engine(case, {"exact_fixup": fix, "exact_min_width": width, "exact_fixup_cap": cap})
    try:
        assert st["iterations"] == iters
        X.assert_parity(X.reference(case), pl, rec, f"{kind} seed {seed} fix {fix} width {width} cap {cap}")
    finally:
        pl.close()


@pytest.mark.gpu
def test_cap_changes_rounds_not_results():
    """A fix-up rollout does reach the cap in the engine: rounds and statistics of a run are a function of its
    decisions, and the only decision the cap changes is that of a fix-up rollout still running at step 48 -- so a run
    with the cap that differs in rounds or statistics from the run without it has stopped one.  The trees are equal."""
    kind, seed, iters = SCENES[0]
    case = _fresh(kind, seed, iters)
    seen = []
    for cap in (0, CAP):
        pl, st, rec = X.run_engine(case, {"exact_fixup_cap": cap})
        try:
            X.assert_parity(X.reference(case), pl, rec, f"cap {cap}")
            seen.append((st["rounds"], pl.exact_stats()))
        finally:
            pl.close()
    print("cap 0:", seen[0], "cap 48:", seen[1])
    assert seen[0] != seen[1]


@pytest.mark.gpu
def test_iteration_log_restarts_between_expands():
    """iteration_log(True) between two expand calls clears the records; the log restarts at the second call's first
    iteration."""
    kind, seed, iters = SCENES[0]
    case = _fresh(kind, seed, iters)
    want = X.reference(case)["records"]
    pl = X.make_planner(case)
    try:
        rng = clrrt.Rng(seed)
        pl.iteration_log(True)
        pl.expand(rng, n_iters=150, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
        assert np.array_equal(X.records(pl), want[:150])
        pl.iteration_log(True)
        assert X.records(pl).shape[0] == 0
        pl.expand(rng, n_iters=iters - 150, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
        rec = X.records(pl)
        assert rec.shape[0] == iters - 150 and np.array_equal(rec, want[150:])
        # without a restart the log runs on; off stops and clears it
        pl.iteration_log(False)
        assert X.records(pl).shape[0] == 0
        X.assert_parity(X.reference(case), pl, want, "two expand calls")
    finally:
        pl.close()


# --------------------------------------------------------------------------------------------- 2. every verdict
# Cases picked from the output of tools/exact_fix_scan.py on an MI355X, with the clrrt_exact_fix_hist each run gave
# there (buckets that were 0 left out).  A run's decisions do not depend on timing, so the counts repeat; a test asserts
# only that its recorded buckets are still reached.
VERDICT_CASES = [
    # none 260, fix_result 16, fix_no_result 31, no_result_pushed_out 23, tie 112, key_eq_thr 2, over_slots 1,
    # recomputed 115, recomputed_stood 106, fixup_succeeded 22, tie_cleared 35
    (("fresh", "obb200", 3, 400, 256, 0, 0),
     ("none", "fix_result", "fix_no_result", "no_result_pushed_out", "tie", "key_eq_thr", "over_slots", "recomputed",
      "recomputed_stood", "fixup_succeeded", "tie_cleared")),
    # none 184, fix_result 6, fix_no_result 88, no_result_pushed_out 63, over_slots 28, recomputed 28,
    # recomputed_stood 27, fixup_succeeded 6
    (("fresh", "moving", 5, 300, 256, 0, 0),
     ("fix_result", "fix_no_result", "no_result_pushed_out", "over_slots", "recomputed_stood", "fixup_succeeded")),
    # none 253, fix_result 8, fix_no_result 1, tie 65, key_eq_thr 5, recomputed 70, recomputed_stood 46,
    # fixup_succeeded 32, tie_cleared 29
    (("fresh", "empty", 3, 300, 256, 0, 0), ("fix_result", "tie", "key_eq_thr", "recomputed_stood", "tie_cleared")),
    # copies of nodes (40 grown iterations + 200 copies): none 172, fix_result 2, fix_no_result 4,
    # no_result_pushed_out 4, tie 160, recomputed 160, recomputed_stood 123, recomputed_stopped 20, fixup_succeeded 18,
    # tie_cleared 38
    (("copies", "obb200", 3, 300, 256, 40, 200),
     ("tie", "recomputed", "recomputed_stood", "recomputed_stopped", "fixup_succeeded", "tie_cleared")),
    # copies on the empty scene (300 grown iterations + 300 copies): none 228, fix_no_result 2, tie 155, recomputed 155,
    # recomputed_stood 70, recomputed_stopped 6, fixup_succeeded 79, tie_cleared 122
    (("copies", "empty", 3, 300, 256, 300, 300),
     ("tie", "recomputed_stood", "recomputed_stopped", "fixup_succeeded", "tie_cleared")),
    # a tree re-initialised from a committed path: none 262, fix_result 10, fix_no_result 34, no_result_pushed_out 12,
    # tie 1, over_slots 1, recomputed 2, recomputed_stood 1, fixup_succeeded 9, tie_cleared 3
    (("replan", "obb200", 11, 300, 256, 300, 0),
     ("fix_result", "fix_no_result", "no_result_pushed_out", "recomputed", "fixup_succeeded", "tie_cleared")),
    # a window of sortLimit 3 (the reference's parameter, 10 in its launch file): the scan met no result pushed out of
    # the window of 10 within 400 iterations of any case above; here none 277, fix_result 10, fix_no_result 22,
    # no_result_pushed_out 19, pushed_out 2, recomputed 2, recomputed_stopped 2, fixup_succeeded 9
    (("fresh", "obb200", 5, 300, 256, 3, 0),
     ("fix_result", "fix_no_result", "no_result_pushed_out", "pushed_out", "recomputed_stopped", "fixup_succeeded")),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,buckets", VERDICT_CASES, ids=["-".join(str(v) for v in c) for c, _ in VERDICT_CASES])
def test_fixup_verdicts_reached_with_parity(case, buckets):
    """Full parity, per-iteration records included, on a run that is shown to take the verdicts recorded for it: a
    later change that silently stops reaching a branch fails here."""
    pl, st, rec = X.run_engine(case)
    try:
        X.assert_parity(X.reference(case), pl, rec, str(case))
        hist = pl.exact_fix_hist()
        print(case, {k: v for k, v in hist.items() if v}, pl.exact_stats())
        missing = [b for b in buckets if hist[b] == 0]
        assert not missing, (missing, hist)
        # the histogram's own arithmetic: one first-level verdict per examined sample; lists are recomputed for
        # unresolved samples only; a recomputed list stands, stops the prefix, or its fix-ups end it
        unresolved = hist["tie"] + hist["key_eq_thr"] + hist["over_slots"] + hist["pushed_out"]
        assert hist["recomputed"] <= unresolved and hist["no_result_pushed_out"] <= hist["fix_no_result"]
        assert hist["recomputed_stood"] + hist["recomputed_stopped"] <= hist["recomputed"]
        assert hist["none"] + hist["fix_result"] + hist["fix_no_result"] + unresolved >= case[3]
    finally:
        pl.close()


def test_verdict_cases_cover_the_buckets():
    """The union of the recorded buckets is every bucket of clrrt_exact_fix_hist but the unreached ones named here.
    (No GPU: it reads the table above.)"""
    reached = set(b for _, bs in VERDICT_CASES for b in bs)
    assert set(clrrt.Planner.EXACT_FIX_BUCKETS) - reached == set(UNREACHED)
    assert len(UNREACHED) <= 2


UNREACHED = ()  # (pushed_out needs the narrow window of the last case: no case with sortLimit 10 reached it)


# --------------------------------------------------------------------------------------------- 3. the 12000 switch
G = 65536  # guard band, as tests/test_capacity_gpu.py


@pytest.fixture
def guarded():
    """Guard bands around every device and pinned block of the planners made in the test body (the fix_* buffers are
    sized from max_batch, the LDS list kernel from 12000 entries); nothing may have written outside its block."""
    X.grown_tree()  # (grown before the guard: not this test's planner)
    clrrt.mem_check()
    clrrt.mem_guard(G)
    made = []
    try:
        yield made
        for pl in made:
            pl.close()
        rep = clrrt.mem_check()
        assert rep["violations"] == 0, rep
        assert rep["blocks_checked"] > 0 and rep["guard_bytes_checked"] == 2 * G * rep["blocks_checked"], rep
    finally:
        for pl in made:
            pl.close()
        clrrt.mem_guard(0)


SWITCH_CASE = ("switch", "obb200", 7, 300, 256, 11900, 0)


@pytest.mark.gpu
def test_exact_across_the_list_kernel_switch(guarded):
    """From 11900 nodes, 300 iterations carry the tree past 12000 nodes: below, k_nn_exact_fused serves the rounds'
    lists and an unresolved sample gets its list recomputed; once the tree and a round's new nodes exceed 12000 the
    lists come from the sort-scratch path and an unresolved sample ends the prefix.  Tree, rows, counters and
    per-iteration records equal the sequential oracle's on both sides of the switch."""
    ref = X.reference(SWITCH_CASE)
    pl, st, rec = X.run_engine(SWITCH_CASE)
    guarded.append(pl)
    X.assert_parity(ref, pl, rec, "across the switch")
    hist, stats = pl.exact_fix_hist(), pl.exact_stats()
    print("switch:", pl.size()[0], "nodes,", st["rounds"], "rounds", hist, stats, pl.search_work())
    assert ref["first_new"] == 11900 and pl.size()[0] > X.SWITCH + 16
    # both list paths ran: lists are recomputed only while tree + new nodes fit 12000 entries ...
    assert hist["recomputed"] > 0
    # ... and past it an unresolved sample ends the prefix instead (end_pushed_out also counts recomputed lists that
    # lost their result, so it is left out of the sum: the three others are counted only past the switch)
    unresolved = hist["tie"] + hist["key_eq_thr"] + hist["over_slots"] + hist["pushed_out"]
    past = stats["end_tie"] + stats["end_key_eq_thr"] + stats["end_over_slots"]
    assert past > 0 and unresolved - hist["recomputed"] >= past
    assert past + stats["end_pushed_out"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("total", [0, 1])
def test_round_at_the_switch_boundary(guarded, total):
    """The round that stands on the switch: the start size is chosen on the CPU, from the oracle's per-iteration
    deltas, so that a first round of two samples that commits both has N + new == 12000 exactly (total 0: the last
    round the LDS kernel serves) or N < 12000 < N + new (total 1: the first round past it).  Then 120 more
    iterations.  Everything equals the oracle's, under guard bands."""
    case2, d = X.boundary_start(20, 256, total)
    case = case2[:3] + (122,) + case2[4:]
    assert case[5] + d == X.SWITCH + total and case[5] < X.SWITCH and d >= 2
    ref = X.reference(case)
    assert int(ref["records"][:2, 0].sum()) == d
    pl = X.make_planner(case)
    guarded.append(pl)
    pl.iteration_log(True)
    rng = clrrt.Rng(case[2])
    st = pl.expand(rng, n_iters=2, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
    # one round, both samples committed: its new nodes are the oracle's d
    assert (st["rounds"], st["iterations"], pl.size()[0]) == (1, 2, X.SWITCH + total), st
    pl.expand(rng, n_iters=120, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
    X.assert_parity(ref, pl, X.records(pl), f"boundary total {total}")
