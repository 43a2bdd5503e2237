"""tests/rebase_ref.py against naive loops (CPU): the doubling closure, its pass count, renumbering, costE'."""
import math

import numpy as np
import pytest

import rebase_ref


def _random_tree(n, seed, chainy=False):
    rng = np.random.default_rng(seed)
    parent = np.full(n, -1, dtype=np.int64)
    for k in range(1, n):
        parent[k] = k - 1 if (chainy and rng.random() < 0.9) else rng.integers(0, k)
    return parent


@pytest.mark.parametrize("n,seed,chainy", [(1, 0, False), (2, 1, False), (200, 2, False), (300, 3, True), (1000, 4, False)])
def test_closure_matches_the_naive_loop(n, seed, chainy):
    parent = _random_tree(n, seed, chainy)
    rng = np.random.default_rng(seed + 100)
    for root in sorted({0, n // 7, n // 2, n - 1}):
        invalid = rng.random(n) < 0.1
        for inv in (None, invalid):
            m, k, lv, passes = rebase_ref.closure(parent, root, inv)
            m2, k2, lv2 = rebase_ref.closure_naive(parent, root, inv)
            assert np.array_equal(m, m2) and np.array_equal(k, k2) and np.array_equal(lv, lv2), (n, root)
            # a member d hops below the root settles in ceil(log2 d) passes; any other node, d hops below node 0, in
            # ceil(log2 (d + 1)) (its last jump goes from node 0 to -1); one more pass moves nothing
            depth_all = rebase_ref.closure_naive(parent, 0)[2]
            longest = max(1, int(np.where(m2, lv2, depth_all + 1).max()))
            assert passes <= math.ceil(math.log2(longest)) + 1, (passes, longest)


def test_chain_of_70_rebased_at_3_takes_7_passes_to_settle():
    parent = np.arange(-1, 69)
    m, k, lv, passes = rebase_ref.closure(parent, 3)
    assert m.sum() == 67 and lv.max() == 66 and not m[:3].any()
    assert passes == 7 + 1  # 66 hops settle in 7 passes; the 8th moves nothing


def test_renumber_and_cost():
    parent = np.array([-1, 0, 0, 1, 1, 2, 3, 3])
    m, k, lv, _ = rebase_ref.closure(parent, 1, np.array([0, 0, 0, 0, 1, 0, 0, 0], dtype=bool))
    assert list(np.flatnonzero(m)) == [1, 3, 4, 6, 7] and list(np.flatnonzero(k)) == [1, 3, 6, 7]
    ids, par = rebase_ref.renumber(k, parent, 1)
    assert list(ids) == [1, 3, 6, 7] and list(par) == [-1, 0, 1, 1]
    ce = rebase_ref.cost_e(np.array([0.0, 1.5, 2.0, 4.25], dtype=np.float32), 1)
    assert list(ce) == [-1.5, 0.0, 0.5, 2.75] and ce.dtype == np.float32
