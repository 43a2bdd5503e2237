"""replan.PlannerBackend(carry_tree=True): three 5 Hz queries that keep their tree (clrrt_tree_rebase) -- GPU."""
import numpy as np
import pytest

import clrrt
from clrrt import abi, replan, scenes

pytestmark = pytest.mark.gpu

B, ROUNDS, SEED = 256, 4, 11
GOAL_W = (40.0, 0.0, 0.0, 0.0)


def _run(kind, carry):
    """(log, per-query (tree size at the start, committed path length before it, rebase info), planner)."""
    mode = abi.CLRRT_COLLISION_STUB if kind == "stub" else abi.CLRRT_COLLISION_OBB
    obs = np.zeros((0, 7)) if kind == "stub" else scenes.urban_scene(200)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), max_nodes=1 << 15, max_rows=1 << 21, max_batch=B)
    make = replan.default_make_params(mode)
    be = replan.PlannerBackend(pl, make) if carry is None else replan.PlannerBackend(pl, make, carry_tree=carry)
    rng = clrrt.Rng(SEED)
    starts = []

    def expand(q):
        n, r = pl.size()
        path_n = pl.path_size()[0]
        free = True
        if carry and be.last_rebase is not None:  # every kept row is free under the query's own check
            free = bool((pl.check_obs_distance(pl.rows(0, r)) != 0).all())
        starts.append((n, path_n, be.last_rebase, free))
        pl.expand(rng, n_iters=B * ROUNDS, mode=clrrt.CLRRT_MODE_BATCH, batch=B)

    log = replan.run_queries(be, expand, 3, obs, goal_world=GOAL_W, v0=1.0)
    return log, starts, pl


@pytest.mark.parametrize("kind", ["stub", "obb200"])
def test_three_queries_carry_their_tree(kind):
    log, starts, pl = _run(kind, True)
    try:
        print(kind, [(n, p, None if i is None else (i["nodes_subtree"], i["nodes_kept"], i["depth"]), f)
                     for n, p, i, f in starts], [len(ids) for _, _, ids in log])
        assert log[0][1] == abi.REINIT_EMPTY and starts[0][0] == 1
        for q in (1, 2):
            n, path_n, info, free = starts[q]
            assert len(log[q - 1][2]) >= 2, (q, "the query before committed no path")
            assert info is not None and info["outcome"] == abi.REBASE_KEPT, (q, info)
            assert log[q][1] == abi.REINIT_KEPT
            assert n == info["nodes_kept"] and n > path_n, (q, n, path_n)
            assert free, q
        # the carried tree still yields a path
        assert len(log[2][2]) >= 2
    finally:
        pl.close()


@pytest.mark.parametrize("kind", ["stub", "obb200"])
def test_carry_off_is_the_existing_sequence(kind):
    a, sa, pa = _run(kind, None)
    b, sb, pb = _run(kind, False)
    try:
        assert [ids for _, _, ids in a] == [ids for _, _, ids in b]
        assert [oc for _, oc, _ in a] == [oc for _, oc, _ in b]
        assert [s[:2] for s in sa] == [s[:2] for s in sb]
        assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))
    finally:
        pa.close()
        pb.close()
