"""The engine at its capacities, under guard bands: trees that fill max_nodes or the row arena, the two capacity exits
of the expansion drivers, trees of exactly max_nodes nodes, and rounds whose size is no power of two -- GPU.

Every context of this module is created with clrrt.mem_guard(G) on: 64 KiB of 0xFF before and after every device and
pinned block, checked when the block is freed and by clrrt.mem_check().  G is more than a super-tile of float4 walk
records (1024 x 16 B) and more than a 256-thread block's worth of clrrt_node headers or trajectory rows, so an overrun
by up to one such unit at the end of a buffer stays inside memory the block itself owns: it is reported, and it
cannot touch a neighbouring block or unmapped memory.  That is why the capacity tests run only with the guard on.

No property here rests on a measured number: each test compares with a roomy context (max_nodes 1 << 16), the CPU
oracle, or the guard's fill pattern.  Trees are grown as tests/test_rebase_gpu.py grows them: BATCH rounds of 256
samples on the 200-obstacle scene, OBB check, with nn_walk_min 64 so that the walk sets serve from small trees on.

Drivers.  A BATCH round always takes `batch` samples (the clock decides only whether a search is prefetched, never a
round's size), so budget queries are reproducible and are used as the issue states them.  nn_lag 0 means "by query
length": lag 2 under the 60 s budget and for 1000 rounds, lag 1 for the roomy contexts' few rounds -- the lists, and
so the trees, are the same under every lag.

nn_range / nn_merge on the full tree: the ranges of a merge must be disjoint (include/clrrt.h), so [0, N) is checked on
its own, and the merge over [0, N - 1) and [N - 1, N).
"""
import re

import numpy as np
import pytest

import clrrt
import query_cases as qc
import walk_cases as wc
from clrrt import abi, replan, scenes
from nn_strategies import nn_strategy
from oracle_binding import Oracle
from test_rebase_gpu import PLACES, Snap, _bits, _box_on, _check, _descendants, _expect
from test_walk_index import STRATEGIES, check_index

pytestmark = pytest.mark.gpu

G = 65536
OBB, STUB = abi.CLRRT_COLLISION_OBB, abi.CLRRT_COLLISION_STUB
BATCH = clrrt.CLRRT_MODE_BATCH
B, SEED = 256, 7
SCENE = scenes.urban_scene(200)
CAP, ROOMY, ROWS = 3001, 1 << 16, 1 << 21
LONG_ROUNDS = 24  # the roomy contexts' long runs: past every capacity stop below (asserted where used)
ECAPACITY = -3


@pytest.fixture
def ctx():
    """The guard is on before any planner exists; the planners a test makes through `ctx` are closed after its body, so
    the checks at free run too; then nothing may have written outside its block."""
    clrrt.mem_check()  # (forget what earlier frees recorded: this test's report is its own)
    clrrt.mem_guard(G)
    made = []
    try:
        yield made
        for pl in made:
            pl.close()
        rep = clrrt.mem_check()
        print(f"guard: {rep['blocks_checked']} blocks, {rep['guard_bytes_checked']} guard bytes checked, "
              f"{rep['violations']} violations")
        assert rep["violations"] == 0, rep
        assert rep["blocks_checked"] > 0 and rep["guard_bytes_checked"] == 2 * G * rep["blocks_checked"], rep
    finally:
        for pl in made:
            pl.close()
        clrrt.mem_guard(0)


def _planner(ctx, max_nodes, max_rows=ROWS, max_batch=B, lag=0, T=0, params=None, obs=SCENE):
    pl = clrrt.Planner(params or clrrt.default_params(collision_mode=OBB), max_nodes=max_nodes, max_rows=max_rows,
                       max_batch=max_batch)
    ctx.append(pl)
    pl.set_option("nn_walk_min", 64)
    pl.set_option("nn_lag", lag)
    pl.set_option("defer_steps", T)
    if obs is not None:
        pl.set_obstacles(obs)
        pl.tree_init()
    return pl


def _rc(e):
    return int(re.search(r"-> (-?\d+)", str(e.value)).group(1))


class Run:
    """What an expansion left: the whole tree, the counters, the returned rng state, the stats, the round sizes."""

    def __init__(self, pl, rng, st=None, counters0=None):
        self.snap = Snap(pl)
        self.n, self.n_rows = pl.size()
        c = pl.counters()
        self.counters = c if counters0 is None else {k: c[k] - counters0[k] for k in c}
        self.rng = bytes(rng.state)
        self.st = st
        self.sizes = pl.round_sizes()

    def assert_same(self, other, label):
        a, b = self.snap, other.snap
        assert (self.n, self.n_rows) == (other.n, other.n_rows), (label, self.n, self.n_rows, other.n, other.n_rows)
        assert bytes(a.raw) == bytes(b.raw), (label, "headers")
        assert np.array_equal(_bits(a.rows), _bits(b.rows)), (label, "rows")
        assert self.counters == other.counters, (label, self.counters, other.counters)
        assert self.rng == other.rng, (label, "rng state")

    def rows_after(self, n):
        """Rows of the first n nodes (rows are appended in node order)."""
        return int(self.snap.nodes["nrows"][:n].sum())


_roomy, _oracles = {}, {}


def roomy(ctx, lag, T, iters, batch=B, seed=SEED):
    """The roomy context's run of `iters` iterations under the same options: once per key, kept as a download."""
    key = (lag, T, iters, batch, seed)
    if key not in _roomy:
        pl = _planner(ctx, ROOMY, max_batch=batch, lag=lag, T=T)
        rng = clrrt.Rng(seed)
        st = pl.expand(rng, n_iters=iters, mode=BATCH, batch=batch)
        assert st["iterations"] == iters and st["capacity_stop"] == 0
        _roomy[key] = Run(pl, rng, st)
    return _roomy[key]


def oracle(T, iters, batch=B, seed=SEED):
    """The oracle's expand_batch(iters, batch, defer_steps=T): once per key, left unchanged."""
    key = (T, iters, batch, seed)
    if key not in _oracles:
        o = Oracle(abi.default_params(collision_mode=OBB), SCENE)
        Oracle.srand(seed)
        o.init_tree()
        ndef = o.expand_batch(iters, batch, stable=True, defer_steps=T, threads=16)
        _oracles[key] = (o, ndef)
    return _oracles[key]


def _rng_after(iters, seed=SEED):
    r = clrrt.Rng(seed)
    for _ in range(3 * iters):
        r.next()
    return bytes(r.state)


def _n_steps_max():
    return qc.n_steps_max(clrrt.default_params(collision_mode=OBB))


def _fill(label, pl, st_rounds, max_nodes, max_rows):
    n, r = pl.size()
    print(f"{label}: {st_rounds} rounds, {n} / {max_nodes} nodes, {r} / {max_rows} rows")


# --------------------------------------------------------------------- (a) budget queries that end on capacity
LAGS_TS = [(lag, T) for lag in (0, 1, 2) for T in (0, 32)]


def _capacity_query(ctx, lag, T):
    pl = _planner(ctx, CAP, lag=lag, T=T)
    rng = clrrt.Rng(SEED)
    st = pl.expand(rng, budget_ms=60000.0, mode=BATCH, batch=B)
    return pl, rng, st


@pytest.mark.parametrize("lag,T", LAGS_TS)
def test_budget_query_ends_on_capacity(ctx, lag, T):
    pl, rng, st = _capacity_query(ctx, lag, T)
    _fill(f"(a) lag {lag} T {T}", pl, st["rounds"], CAP, ROWS)
    assert st["capacity_stop"] == 1, st
    assert st["iterations"] == st["rounds"] * B and st["rounds"] >= 4, st
    n, r = pl.size()
    assert n <= CAP and r <= ROWS and st["nodes_added"] == n - 1
    got = Run(pl, rng, st)
    assert got.rng == _rng_after(st["iterations"])
    ref = roomy(ctx, lag, T, st["iterations"])
    got.assert_same(ref, f"lag {lag} T {T} vs roomy")
    assert st["deferred"] == ref.st["deferred"] and st["goal_nodes_added"] == ref.st["goal_nodes_added"]
    o, ndef = oracle(T, st["iterations"])
    assert (ndef > 0) == (T > 0) and st["deferred"] == ndef
    qc.assert_tree_equal(o, pl, f"lag {lag} T {T} vs oracle")
    if T == 0:
        # the documented rule, restated: a round runs while n + 2 B <= max_nodes (and likewise for the arena's rows,
        # which must not be what stopped this query): every round that ran was due, and the next one is not
        sizes = [int(v) for v in ref.sizes]
        assert len(sizes) == st["rounds"]
        before = [1] + sizes[:-1]
        assert all(nb + 2 * B <= CAP for nb in before), "a round ran that the rule refuses"
        assert sizes[-1] + 2 * B > CAP, "the query stopped a round early"
        assert ref.n_rows + 2 * B * (_n_steps_max() + 1) <= ROWS


# --------------------------------------------------------------------------------- (b) the arena as the limit
def _arena_case(ctx, lag):
    """(max_rows, rounds that fit, the roomy run of that many rounds) for the arena-limited context."""
    long = roomy(ctx, lag, 0, LONG_ROUNDS * B)
    sizes = [int(v) for v in long.sizes]
    k = 6
    while long.rows_after(sizes[k]) - long.rows_after(sizes[k - 1]) <= 7:  # the next round must add more than 7 rows
        k += 1
    assert k + 2 < LONG_ROUNDS
    rk, rk1 = long.rows_after(sizes[k - 1]), long.rows_after(sizes[k])
    assert rk1 - rk > 7
    return rk + 2 * B * (_n_steps_max() + 1) + 7, k + 1, rk1


@pytest.mark.parametrize("lag", [1, 2])
def test_arena_is_the_limit(ctx, lag):
    max_rows, rounds, rows_then = _arena_case(ctx, lag)
    pl = _planner(ctx, ROOMY, max_rows=max_rows, lag=lag)
    rng = clrrt.Rng(SEED)
    st = pl.expand(rng, budget_ms=60000.0, mode=BATCH, batch=B)
    _fill(f"(b) lag {lag}", pl, st["rounds"], ROOMY, max_rows)
    assert st["capacity_stop"] == 1 and st["rounds"] == rounds == 7 and st["iterations"] == rounds * B, (st, rounds)
    assert pl.size()[1] == rows_then <= max_rows
    Run(pl, rng, st).assert_same(roomy(ctx, lag, 0, rounds * B), f"arena, lag {lag}")
    qc.assert_tree_equal(oracle(0, rounds * B)[0], pl, f"arena, lag {lag} vs oracle")


# ------------------------------------------------------------------------ (c) an iteration count past capacity
@pytest.mark.parametrize("lag,T,arena", [(lag, T, False) for lag, T in LAGS_TS] + [(1, 0, True), (2, 0, True)])
def test_iteration_count_past_capacity(ctx, lag, T, arena):
    """With deferred samples this is also the regression test of the refusal's row bookkeeping: the replays the step
    cap had suspended (rows owed to committed nodes) were dropped with the abandoned samples' chains, and the tails
    of those nodes' trajectories stayed zero in the arena."""
    max_nodes, max_rows = (ROOMY, _arena_case(ctx, lag)[0]) if arena else (CAP, ROWS)
    pl = _planner(ctx, max_nodes, max_rows=max_rows, lag=lag, T=T)
    rng = clrrt.Rng(SEED)
    with pytest.raises(clrrt.ClrrtError) as e:
        pl.expand(rng, n_iters=1000 * B, mode=BATCH, batch=B)
    assert _rc(e) == ECAPACITY and "tree capacity exhausted" in str(e.value), str(e.value)
    n, r = pl.size()
    long = roomy(ctx, lag, T, LONG_ROUNDS * B)
    sizes = [int(v) for v in long.sizes[:LONG_ROUNDS]]
    assert n in sizes and sizes.index(n) < LONG_ROUNDS - 1, (n, sizes)  # the roomy run passed it
    k = sizes.index(n) + 1
    print(f"(c) lag {lag} T {T} arena {arena}: refused after {k} rounds, {n} / {max_nodes} nodes, {r} / {max_rows} rows")
    assert k >= 4 and n <= max_nodes and r <= max_rows
    assert bytes(rng.state) == _rng_after(k * B)
    # the nodes and rows present are that prefix of the roomy tree
    assert r == long.rows_after(n)
    sz = len(bytes(long.snap.raw)) // long.n
    assert bytes(pl.nodes_raw()) == bytes(long.snap.raw)[:n * sz]
    assert np.array_equal(_bits(pl.rows(0, r)), _bits(long.snap.rows[:r]))
    if T > 0:  # the expansion was abandoned with samples pending in the deferral rings
        assert long.st["deferred"] > 0
        o_n = oracle(T, k * B)[0].size()  # (the oracle drains at its end: what was pending makes the difference)
        assert o_n > n, "no sample was pending when the expansion was refused"
    # the next query on the same context: nothing of the abandoned expansion leaks into it
    c0 = pl.counters()
    pl.tree_init()
    rng2 = clrrt.Rng(99)
    st2 = pl.expand(rng2, n_iters=3 * B, mode=BATCH, batch=B)
    assert st2["rounds"] == 3 and st2["capacity_stop"] == 0
    again = Run(pl, rng2, st2, counters0=c0)
    fresh = _planner(ctx, max_nodes, max_rows=max_rows, lag=lag, T=T)
    rng3 = clrrt.Rng(99)
    st3 = fresh.expand(rng3, n_iters=3 * B, mode=BATCH, batch=B)
    again.assert_same(Run(fresh, rng3, st3), f"after the refused expansion, lag {lag} T {T}")
    assert {k2: st2[k2] for k2 in st2 if k2 != "elapsed_ms"} == {k2: st3[k2] for k2 in st3 if k2 != "elapsed_ms"}


# --------------------------------------------------------------------- (d) a tree of exactly max_nodes nodes
def _full_tree(N):
    if N == wc.N_MAIN:
        rec, groups = wc.main_tree()
        return rec, wc.finite_for_oracle(rec, groups), groups
    rec = wc.small_tree(N)
    return rec, rec, None


def _full_samples(rec, groups, feas_len):
    if groups is not None:
        x, y, ex, _ = wc.samples(rec, groups, feas_len)
        return x, y, ex
    rng = np.random.default_rng(len(rec["x"]))
    n = 96  # uniform over the sample region, and 16 at a node's ref.back() point
    x, y = rng.uniform(-1.9, 51.9, n), rng.uniform(-8.9, 8.9, n)
    at = rng.integers(0, len(rec["x"]), 16)
    x[:16], y[:16] = rec["bx"][at], rec["by"][at]
    return x, y, (np.arange(n) % 4 < 2).astype(np.int32)


def _stub_planner(ctx, max_nodes, rec):
    pl = _planner(ctx, max_nodes, max_rows=1 << 16, params=clrrt.default_params(collision_mode=STUB), obs=None)
    pl.set_option("nn_walk_min", 0)
    pl.tree_load(wc.nodes_raw(rec))
    return pl


@pytest.mark.parametrize("N", [33, 1023, 1024, 1025, wc.N_MAIN])
def test_tree_of_exactly_max_nodes(ctx, N):
    rec, rec_o, groups = _full_tree(N)
    big = _stub_planner(ctx, 1 << 13, rec)
    pl = _stub_planner(ctx, N, rec)
    assert pl.size()[0] == N
    x, y, ex = _full_samples(rec, groups, 2.1 * pl.params.ref_res)
    smp = wc.sample_structs(x, y, ex)
    # every walk strategy's lists against the brute force's on the roomy planner
    nn_strategy(big, "brute")
    ib, kb = big.sort_nodes_batch(smp, exact=False)
    assert (ib >= 0).any(axis=1).sum() > len(smp) // 2
    for strategy in STRATEGIES + ["brute"]:
        nn_strategy(pl, strategy)
        iw, kw = pl.sort_nodes_batch(smp, exact=False)
        bad = np.nonzero((ib != iw).any(axis=1) | (_bits(kb) != _bits(kw)).any(axis=1))[0]
        assert bad.size == 0, (N, strategy, bad[:8], ib[bad[0]], iw[bad[0]])
    nn_strategy(pl, "walk")
    # the index of the full tree
    bad = check_index(pl.walk_index(), rec)
    assert bad == [], bad
    bad = check_index(pl.walk_index(fused=False, first=N - 1, count=1), rec)
    assert bad == [], bad
    # range lists: the whole tree as one range, and the last node as a range of its own
    listed = ib >= 0
    ids0, keys0, cnt0 = pl.nn_range(smp, 0, N)
    assert np.array_equal(cnt0, listed.sum(axis=1)) and np.array_equal(ids0, ib)
    assert np.array_equal(_bits(keys0)[listed], _bits(kb)[listed])
    parts = [pl.nn_range(smp, 0, N - 1), pl.nn_range(smp, N - 1, 1)]
    last = parts[1]
    assert set(np.unique(last[0])) <= {-1, N - 1} and (last[2] <= 1).all()
    ids, keys, cnt = pl.nn_merge(*[np.stack([q[i] for q in parts]) for i in range(3)])
    assert np.array_equal(cnt, cnt0) and np.array_equal(ids, ib), N
    assert np.array_equal(_bits(keys)[listed], _bits(kb)[listed])
    in_list = (ib == N - 1).any(axis=1)
    assert (last[2][in_list] == 1).all()  # a listed node is feasible in its own range too
    # the oracle-finite samples: no NaN key among the tree's nodes (std::stable_sort has no order for one)
    S = np.repeat(np.stack([x, y], axis=1), N, axis=0)
    tile = lambda v: np.tile(np.asarray(v, np.float64), len(x))  # noqa: E731
    keyed = big.selftest_units(abi.UNIT_DUBINS, np.column_stack([S, tile(rec_o["x"]), tile(rec_o["y"]), tile(rec_o["h"]),
                                                                  tile(rec_o["ce"])]))
    finite = ~np.isnan(keyed[:, :2]).reshape(len(x), N, 2).any(axis=(1, 2))
    pick = np.nonzero(finite)[0][:32]
    assert pick.size >= 24
    pl.tree_load(wc.nodes_raw(rec_o))
    o = Oracle(abi.default_params(collision_mode=STUB), None)
    o.load_tree(wc.nodes_raw(rec_o))
    iw, kw = pl.sort_nodes_batch([smp[q] for q in pick], exact=False)
    for j, q in enumerate(pick):
        oi, ok = o.sort_nodes(smp[q].x, smp[q].y, smp[q].explore, stable=True)
        k = min(len(oi), 10)
        assert list(iw[j][:k]) == oi[:k] and (iw[j][k:] == -1).all(), (N, q, oi, iw[j])
        assert np.array_equal(_bits(kw[j][:k]), _bits(np.array(ok[:k], np.float32))), (N, q)
    # every node a goal node, costs tied over 3 values: goal_recs and bp_path at max_nodes entries
    raw = wc.nodes_raw(rec_o)
    rs = np.random.default_rng(N)
    for i in range(N):
        raw[i].goal, raw[i].costS = 1, 3.0 + 0.5 * float(rs.integers(0, 3))
    pl.tree_load(raw)
    o.load_tree(raw)
    path, cost, ng = pl.extract_best_path()
    assert ng == N and path == o.extract_best_path() and np.float32(cost) == np.float32(raw[path[-1]].costS)
    # no round fits: refused, the tree untouched
    before = bytes(pl.nodes_raw())
    c0 = pl.counters()
    with pytest.raises(clrrt.ClrrtError) as e:
        pl.expand(clrrt.Rng(3), n_iters=B, mode=BATCH, batch=B)
    assert _rc(e) == ECAPACITY and "tree capacity exhausted" in str(e.value)
    assert pl.size()[0] == N and bytes(pl.nodes_raw()) == before and pl.counters() == c0


# ------------------------------------------------------------- (e) the ops that follow a query, on the full tree
def test_ops_after_a_capacity_stop(ctx):
    lag, T = 2, 32
    pl, rng, st = _capacity_query(ctx, lag, T)
    assert st["capacity_stop"] == 1
    iters = st["iterations"]
    o = oracle(T, iters)[0]
    # extractBestPath and the committed path
    path, cost, ng = pl.extract_best_path()
    on = o.nodes()
    assert ng == int(on["goal"].sum()) > 0 and path == o.extract_best_path() and len(path) >= 2
    assert pl.path_commit(path) == 0
    o.path_commit(path)
    praw, prows = pl.path_download()
    oraw = o.path_nodes()
    assert len(praw) == len(oraw) == len(path)
    gp, op = clrrt.nodes_to_numpy(praw), clrrt.nodes_to_numpy(oraw)
    for k in ("state", "ref_front", "ref_back", "ref_vback", "ang_par", "costE", "costS"):
        assert np.array_equal(_bits(gp[k]), _bits(op[k])), k
    for k in ("parent", "goal", "nrows"):
        assert np.array_equal(gp[k], op[k]), k
    assert np.array_equal(_bits(prows), _bits(np.concatenate([o.path_rows(i) for i in range(len(path))])))
    # the same tree in a roomy context, to continue beside this one
    room = _planner(ctx, ROOMY, lag=lag, T=T)
    rng_r = clrrt.Rng(SEED)
    room.expand(rng_r, n_iters=iters, mode=BATCH, batch=B)
    assert bytes(rng_r.state) == bytes(rng.state)
    # tree_rebase at node 0 with a small oblique pose: every scratch buffer is sized by the full tree.  A box on a node
    # with many descendants (the reference decides what it takes) makes room for further rounds.
    snap = Snap(pl)
    pose = (0.4, -0.2, 0.05)
    ref = _planner(ctx, 1 << 14, obs=None)
    nd = snap.nodes
    cnt = _descendants(nd["parent"])
    base = replan.obstacles_in_car_frame(SCENE, 0.0, pose)
    ref.set_obstacles(base)
    e0 = _expect(snap, 0, pose, 0.0, ref)
    assert not e0["root_collides"]
    e = None
    for victim in [int(v) for v in np.argsort(-cnt)[1:9] if nd["nrows"][v] >= 3]:
        vi = int(np.flatnonzero(e0["ids"] == victim)[0]) if victim in e0["ids"] else -1
        if vi < 0:
            continue
        mid = e0["rows"][e0["row_offset"][vi] + e0["nrows"][vi] // 2]
        for place in PLACES:
            obs = np.vstack([base, np.asarray(_box_on(mid, **place), dtype=np.float64).reshape(1, 7)])
            ref.set_obstacles(obs)
            e = _expect(snap, 0, pose, 0.0, ref)
            if not e["root_collides"] and 64 <= e["nodes_kept"] <= CAP - 2 * B:
                break
        else:
            continue
        break
    # (n + 2 B <= max_nodes: at least one more round fits)
    assert e is not None and not e["root_collides"] and 64 <= e["nodes_kept"] <= CAP - 2 * B, "no box leaves room"
    for p in (pl, room):
        p.set_obstacles(obs)
    info = pl.tree_rebase(0, pose, 0.0)
    print(f"(e) rebase of the {snap.n}-node tree: {info}")
    _check(pl, info, e, "full tree")
    info_r = room.tree_rebase(0, pose, 0.0)
    assert {k: v for k, v in info.items() if k != "device_ms"} == {k: v for k, v in info_r.items() if k != "device_ms"}
    # a further budget query on the carried tree stops on capacity again, as the roomy context's continuation
    c0, c0r = pl.counters(), room.counters()
    rng2 = clrrt.Rng(11)
    st2 = pl.expand(rng2, budget_ms=60000.0, mode=BATCH, batch=B)
    _fill("(e) the query on the carried tree", pl, st2["rounds"], CAP, ROWS)
    assert st2["capacity_stop"] == 1 and st2["rounds"] >= 1 and st2["iterations"] == st2["rounds"] * B
    assert pl.size()[0] <= CAP
    rng2r = clrrt.Rng(11)
    st2r = room.expand(rng2r, n_iters=st2["iterations"], mode=BATCH, batch=B)
    Run(pl, rng2, st2, c0).assert_same(Run(room, rng2r, st2r, c0r), "the carried tree's query")


# ------------------------------------------------------------------------------- (f) odd and partial rounds
ODD = [(b, 4 * b, b) for b in (1, 63, 65, 257)] + [(B, 3 * B + 1, B), (B, 3 * B + 255, B)]


@pytest.mark.parametrize("lag", [0, 2])
@pytest.mark.parametrize("T", [0, 32])
@pytest.mark.parametrize("max_batch,n,b", ODD)
def test_odd_and_partial_rounds(ctx, max_batch, n, b, T, lag):
    pl = _planner(ctx, ROOMY, max_batch=max_batch, lag=lag, T=T)
    rng = clrrt.Rng(SEED)
    st = pl.expand(rng, n_iters=n, mode=BATCH, batch=b)
    assert st["iterations"] == n and st["rounds"] == 4 and st["capacity_stop"] == 0, st
    assert bytes(rng.state) == _rng_after(n)
    o, ndef = oracle(T, n, batch=b)
    assert st["deferred"] == ndef
    qc.assert_tree_equal(o, pl, f"batch {b} n {n} T {T} lag {lag}")


# ---------------------------------------------------------------------------------------- (g) the guard is live
def test_guard_is_live(ctx):
    pl = _planner(ctx, CAP)
    pl.expand(clrrt.Rng(SEED), n_iters=2 * B, mode=BATCH, batch=B)
    live = clrrt.mem_check()  # the context's blocks (and the scratch blocks freed so far)
    assert live["violations"] == 0 and live["guard_bytes_checked"] == 2 * G * live["blocks_checked"]
    pl.close()
    held = clrrt.mem_check()  # what the owner held: each block was checked at its free
    print(f"(g) {live['blocks_checked']} blocks checked beside the live context, {held['blocks_checked']} freed by its owner")
    assert held["violations"] == 0 and held["guard_bytes_checked"] == 2 * G * held["blocks_checked"]
    assert live["blocks_checked"] >= held["blocks_checked"] >= 3  # (the tree, its search records, the arena, ...)
    # a guard that is off hands out unguarded blocks: nothing to check
    clrrt.mem_guard(0)
    un = _planner(ctx, CAP)
    assert clrrt.mem_check()["blocks_checked"] == 0
    un.close()
    for bad in (1, 255, 1000, (1 << 20) + 256, -256):
        with pytest.raises(clrrt.ClrrtError):
            clrrt.mem_guard(bad)
    clrrt.mem_guard(G)
    _planner(ctx, CAP)  # (the fixture's closing check wants a guarded block)
