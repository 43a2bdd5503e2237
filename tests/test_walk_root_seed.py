"""Root seed of the walk search (option nn_root_seed, clrrt_nnwalk.hip) -- GPU.

An optimize sample's walk starts from the roster: the first copies of the root pose by id (the root and its
zero-length children, which all share one key for a sample), decided by the search's own feasibleNode.  The seed
only changes the work: every list must equal the brute force's, and every tree the unseeded walk's.

Lists are compared through clrrt_nn_batch: the 10 (key bits, id) pairs it returns in BATCH order, and again in EXACT
order, whose re-sort of tied samples is driven by the tie flag the 11th pair decides.
"""
import numpy as np
import pytest

import clrrt
from clrrt import abi, scenes
from clrrt import dist as cdist

pytestmark = pytest.mark.gpu

NOPT = NEXP = 256
RING = 3.0  # radius of the root copies' ref.back() ring [m]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _walk(pl, seed=1, split=False, **opts):
    """The walk for trees of any size (the _nn_strategy settings of test_gpu_parity.py); split: a budget of one tile,
    so every sample hands its search to the overflow split."""
    pl.set_option("nn_exact_fused", 0)
    pl.set_option("nn_walk_min", 0)
    pl.set_option("nn_walk_waves", 0)
    pl.set_option("nn_walk_budget_tiles", 1 if split else 2048)
    pl.set_option("nn_walk_budget_keys", 1 if split else 4096)
    pl.set_option("nn_walk_chunks", 7 if split else 16)
    pl.set_option("nn_walk_max_over", 1024)
    pl.set_option("nn_root_seed", seed)
    for k, v in opts.items():
        pl.set_option(k, v)


def _brute(pl):
    pl.set_option("nn_exact_fused", 0)
    pl.set_option("nn_walk_min", 1 << 40)


def _synthetic(copies, n_other=3000, late=0, seed=5):
    """A tree of the root, `copies` copies of its pose (same x, y, heading, costE 0) at ids 1, 4, 7, ... whose
    ref.back() points lie on a ring around it (ang_par in [-60, 60] degrees, so a sample behind the root has no
    feasible copy), `late` more copies at the end of the id range, and n_other
    ordinary nodes; every 100th of those is cheap (costE half its distance from the root, heading away from it), so
    an optimize sample just ahead of it prefers it to the root."""
    rs = np.random.RandomState(seed)
    n = 1 + n_other + copies + late
    nodes = (abi.Node * n)()
    copy_ids = set(1 + 3 * i for i in range(copies)) | set(range(n - late, n))
    assert max(copy_ids, default=0) < n
    cheap = []
    k = 0
    for i in range(n):
        d = nodes[i]
        d.parent = -1 if i == 0 else 0
        if i == 0:
            d.ref_front[0], d.ref_front[1] = -1.0, 0.0
            d.ang_par = 0.0
            continue
        if i in copy_ids:
            phi = np.deg2rad(-60.0 + 120.0 * ((k * 0.6180339887) % 1.0))
            k += 1
            d.ref_back[0], d.ref_back[1] = RING * np.cos(phi), RING * np.sin(phi)
            d.ref_vback = 1.0
            d.ang_par = float(np.arctan2(d.ref_back[1], d.ref_back[0]))
            continue
        x, y = rs.uniform(0.5, 50.0), rs.uniform(-8.0, 8.0)
        th = np.arctan2(y, x) + rs.uniform(-0.3, 0.3)
        dist = float(np.hypot(x, y))
        d.state[0], d.state[1], d.state[2] = x, y, th
        d.ref_back[0], d.ref_back[1] = x, y
        d.ref_front[0], d.ref_front[1] = x - np.cos(th), y - np.sin(th)
        d.ang_par = float(th)
        d.costE = np.float32(2.0 + dist * rs.uniform(1.3, 2.0))
        if i % 100 == 0:
            d.state[2] = d.ang_par = float(np.arctan2(y, x))
            d.ref_front[0], d.ref_front[1] = x - np.cos(d.ang_par), y - np.sin(d.ang_par)
            d.costE = np.float32(0.5 * dist)
            cheap.append((x, y, d.ang_par))
    return nodes, cheap


def _samples(cheap, seed=9):
    """256 optimize + 256 explore samples: random ones around the tree, 48 behind the root, and 24 optimize samples
    3.5 m ahead of cheap nodes."""
    rs = np.random.RandomState(seed)
    out = []
    for ex in (0, 1):
        pts = [(rs.uniform(-5.0, 55.0), rs.uniform(-12.0, 12.0)) for _ in range(NOPT - 48 - (24 if not ex else 0))]
        pts += [(rs.uniform(-15.0, -5.0), rs.uniform(-4.0, 4.0)) for _ in range(48)]
        if not ex:
            pts += [(x + 3.5 * np.cos(a), y + 3.5 * np.sin(a)) for x, y, a in cheap[:24]]
        assert len(pts) == NOPT
        out += [abi.Sample(float(x), float(y), ex, 0) for x, y in pts]
    return out


def _planner(nodes, sort_limit=10, max_nodes=1 << 13):
    p = clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_STUB)
    p.sort_limit = sort_limit
    pl = clrrt.Planner(p, max_nodes=max_nodes, max_rows=1 << 16, max_batch=NOPT + NEXP)
    pl.tree_load(nodes)
    return pl


def _lists(pl, smp):
    return [pl.sort_nodes_batch(smp, exact=e) for e in (False, True)]


def _assert_lists_equal(ref, got, what):
    for (ib, kb), (iw, kw), order in zip(ref, got, ("BATCH", "EXACT")):
        bad = np.nonzero((ib != iw).any(axis=1) | (_bits(kb) != _bits(kw)).any(axis=1))[0]
        assert bad.size == 0, f"{what}, {order} order: samples {bad[:8]} differ, e.g. {ib[bad[0]]} vs {iw[bad[0]]}"


_CACHE = {}


def _case(copies, sort_limit=10, late=0):
    """(tree, samples, brute-force lists) of a synthetic tree, computed once."""
    key = (copies, sort_limit, late)
    if key not in _CACHE:
        nodes, cheap = _synthetic(copies, late=late)
        smp = _samples(cheap)
        pl = _planner(nodes, sort_limit)
        try:
            _brute(pl)
            _CACHE[key] = (nodes, smp, _lists(pl, smp))
        finally:
            pl.close()
    return _CACHE[key]


def _check_reference(copies, ref, smp):
    """The reference lists show what the cases are for."""
    ids = ref[0][0]
    opt, ahead, behind = slice(0, NOPT), slice(NOPT - 24, NOPT), slice(NOPT - 72, NOPT - 24)
    is_copy = (ids >= 1) & (ids <= 1 + 3 * (copies - 1)) & ((ids - 1) % 3 == 0) | (ids == 0)
    assert (is_copy[opt] & (ids[opt] >= 0)).any(axis=1).sum() > 64  # optimize lists hold root copies
    assert not is_copy[behind].any()  # behind the root no copy is feasible
    assert (~is_copy[ahead][:, 0] & (ids[ahead][:, 0] > 0)).sum() > 12  # a cheap node beats the root's key


@pytest.mark.parametrize("copies", [5, 11, 12, 63, 64, 65, 300])
def test_synthetic_lists_match_brute_force(copies):
    nodes, smp, ref = _case(copies)
    _check_reference(copies, ref, smp)
    pl = _planner(nodes)
    try:
        _walk(pl)
        pl.reset_counters()
        got = _lists(pl, smp)
        d = pl.debug_counters()
        print(f"{copies} copies: optimize samples whose list is the seeded list {d[27]}, seeded short {d[63]} "
              f"(of {2 * NOPT} optimize searches), exact keys {pl.search_work()['exact_keys']}")
        _assert_lists_equal(ref, got, f"{copies} copies")
        assert d[27] + d[63] > 0  # the seed ran
        if copies + 1 < 11:
            assert d[63] == 2 * NOPT  # root and copies are fewer than NN_K: every optimize sample is seeded short
    finally:
        pl.close()


def test_sort_limit_four():
    nodes, smp, ref = _case(64, sort_limit=4)
    assert ((ref[0][0] >= 0).sum(axis=1) <= 4).all() and ((ref[0][0] >= 0).sum(axis=1) == 4).any()
    pl = _planner(nodes, sort_limit=4)
    try:
        _walk(pl)
        _assert_lists_equal(ref, _lists(pl, smp), "sort_limit 4")
    finally:
        pl.close()


@pytest.mark.parametrize("scan,k", [(512, 16), (512, 4), (1, 1)])
def test_copies_past_the_scan_limit(scan, k):
    """6 copies at ids 1 .. 16 and 200 appended last (ids > 3000): the roster ends at the scan limit (or at its K
    entries) and the walk finds the copies beyond it as before."""
    nodes, smp, ref = _case(6, late=200)
    late = (ref[0][0] > 3000).any(axis=1)[:NOPT].sum()
    print(f"optimize lists holding a late copy: {late}")
    assert late > 32
    pl = _planner(nodes)
    try:
        _walk(pl, nn_root_scan=scan, nn_root_k=k)
        _assert_lists_equal(ref, _lists(pl, smp), f"scan {scan}, K {k}")
    finally:
        pl.close()


@pytest.mark.parametrize("copies", [12, 300])
def test_every_sample_through_the_overflow_split(copies):
    nodes, smp, ref = _case(copies)
    pl = _planner(nodes)
    try:
        _walk(pl, split=True)
        pl.reset_counters()
        got = pl.sort_nodes_batch(smp, exact=False)
        records = pl.debug_counters()[32]
        print(f"{copies} copies: overflow records {records} of {len(smp)} samples")
        assert records > 0  # (a sample whose seeded walk visits at most one tile stays inside the budget)
        _assert_lists_equal(ref[:1], [got], f"split, {copies} copies")
    finally:
        pl.close()


def _grow(batch, rounds, seed, **opts):
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=1 << 15,
                       max_rows=1 << 25, max_batch=batch)
    try:
        _walk(pl, seed=seed, nn_walk_budget_tiles=8, nn_walk_budget_keys=32, **opts)
        pl.set_obstacles(scenes.urban_scene(200))
        pl.tree_init()
        st = pl.expand(clrrt.Rng(12), n_iters=batch * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
        assert st["rounds"] == rounds
        n, nr = pl.size()
        return n, bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), pl.debug_counters()
    finally:
        pl.close()


@pytest.mark.parametrize("batch,rounds", [(96, 8), (2048, 5)])
@pytest.mark.parametrize("defer", [0, 128])
def test_trees_equal_with_and_without_seed(batch, rounds, defer):
    """BATCH rounds (lag-2 pipeline, small budgets so some samples overflow) grow the same tree byte for byte."""
    off = _grow(batch, rounds, 0, nn_lag=2, defer_steps=defer)
    on = _grow(batch, rounds, 1, nn_lag=2, defer_steps=defer)
    print(f"{batch} x {rounds}, defer_steps {defer}: {on[0]} nodes; seeded-list samples {on[3][27]}, seeded short "
          f"{on[3][63]}, overflow records {off[3][32]} -> {on[3][32]}")
    assert on[0] == off[0] and on[0] > rounds
    assert on[1] == off[1] and on[2] == off[2]
    assert off[3][27] == 0 and off[3][63] == 0 and on[3][27] + on[3][63] > 0
    if batch == 2048:
        assert off[3][32] > 0  # the overflow hand-over ran beside the seed


def test_partitioned_search_two_ranks():
    """W = 2 (clrrt_nn_range / clrrt_nn_merge): rank 0's range starts at the root and uses the roster, rank 1's does
    not; parts and merged lists equal the unseeded ones."""
    nodes, smp, ref = _case(300)
    res = {}
    for seed in (0, 1):
        pl = _planner(nodes)
        try:
            _walk(pl, seed=seed)
            N = pl.size()[0]
            parts = [pl.nn_range(smp, *cdist.node_range(N, 2, r)) for r in range(2)]
            res[seed] = (parts, pl.nn_merge(*[np.stack([q[i] for q in parts]) for i in range(3)]))
        finally:
            pl.close()
    for (i0, k0, c0), (i1, k1, c1) in zip(res[0][0] + [res[0][1]], res[1][0] + [res[1][1]]):
        assert np.array_equal(i0, i1) and np.array_equal(c0, c1) and np.array_equal(_bits(k0), _bits(k1))
    ids, keys, cnt = res[1][1]
    assert np.array_equal(ids, ref[0][0])
    used = np.arange(10)[None, :] < cnt[:, None]
    assert np.array_equal(_bits(keys)[used], _bits(ref[0][1])[used])


def test_reinit_from_committed_path_then_a_round():
    """initializeTree from a committed path replaces the tree (and its root): the next searches' roster follows it."""
    obs = scenes.urban_scene(50)
    out = {}
    for seed in (0, 1):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=1 << 14,
                           max_rows=1 << 21, max_batch=512)
        try:
            pl.set_obstacles(obs)
            pl.tree_init()
            pl.expand(clrrt.Rng(4), n_iters=250, mode=clrrt.CLRRT_MODE_EXACT, batch=256)
            _walk(pl, seed=seed)
            smp = list(clrrt.Rng(8).draw_samples(pl.params, 512))
            pl.sort_nodes_batch(smp, exact=False)  # an index (and roster) of the old tree
            ids = pl.extract_best_path()[0]
            assert ids and pl.path_commit(ids) == 0
            assert pl.tree_init_from_path([0, 0, 0, 0.05, 1.5, 0.1]) == abi.REINIT_KEPT
            n0 = pl.size()[0]
            walked = pl.sort_nodes_batch(smp, exact=False)
            pl.expand(clrrt.Rng(5), n_iters=2 * 512, mode=clrrt.CLRRT_MODE_BATCH, batch=512)
            after = pl.sort_nodes_batch(smp, exact=False)
            n, nr = pl.size()
            _brute(pl)
            _assert_lists_equal([pl.sort_nodes_batch(smp, exact=False)], [after], f"after the rounds, seed {seed}")
            out[seed] = (n0, walked, n, bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes())
        finally:
            pl.close()
    print(f"re-initialised tree {out[1][0]} nodes, {out[1][2]} after two rounds")
    assert 1 < out[1][0] < out[1][2]
    _assert_lists_equal([out[0][1]], [out[1][1]], "re-initialised tree")
    assert out[0][2:] == out[1][2:]
