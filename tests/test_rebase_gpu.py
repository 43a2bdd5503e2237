"""clrrt_tree_rebase (include/clrrt.h): the tree carried across replanning queries -- GPU, 0 ulp throughout.

Trees are grown with BATCH, 256 samples x 4 rounds, on the 200-obstacle scene (as tests/query_cases.py grows its
trees).  tests/rebase_ref.py restates the bookkeeping (closure, renumbering, costE', the row heading / time
subtractions); everything else is pinned by the engine's own entries on a second planner: path_load + path_transform
+ path_download for header and row (x, y) bits, clrrt_obstacle_distance on the transformed rows for validity,
tree_init_from_path on loaded chains for costS' and goal.
"""
import ctypes as C

import numpy as np
import pytest

import clrrt
import rebase_ref
from clrrt import abi, replan, scenes
from nn_strategies import nn_strategy

pytestmark = pytest.mark.gpu

OBB, OCC, STUB = abi.CLRRT_COLLISION_OBB, abi.CLRRT_COLLISION_OCC, abi.CLRRT_COLLISION_STUB
B, ROUNDS, SEED = 256, 4, 7
SCENE = scenes.urban_scene(200)
POSE = (3.1, -0.7, 0.3)  # oblique


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def _planner(params=None):
    return clrrt.Planner(params or clrrt.default_params(collision_mode=OBB), max_nodes=1 << 14, max_rows=1 << 21,
                         max_batch=B)


def _grow(pl, rounds=ROUNDS):
    pl.set_obstacles(SCENE)
    pl.tree_init()
    pl.expand(clrrt.Rng(SEED), n_iters=B * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=B)


class Snap:
    """A download of the whole tree: raw headers, their numpy view, every row."""

    def __init__(self, pl, n=None):
        nn, nr = pl.size()
        self.raw = pl.nodes_raw()
        self.rows = pl.rows(0, nr)
        self.nodes = clrrt.nodes_to_numpy(self.raw)
        self.n = nn if n is None else n
        if n is not None:
            self.nodes = {k: v[:n] for k, v in self.nodes.items()}

    def same_as(self, other):
        return bytes(self.raw) == bytes(other.raw) and np.array_equal(_bits(self.rows), _bits(other.rows))


def _scene_in(pose, extra=None):
    o = replan.obstacles_in_car_frame(SCENE, 0.0, pose)
    return o if extra is None else np.vstack([o, np.asarray(extra, dtype=np.float64).reshape(-1, 7)])


_ref = {}


def _ref_planner(params, obs, grid=None, clear_max=0.0):
    """The second planner that computes the references, configured like the planner under test."""
    if "pl" not in _ref:
        _ref["pl"] = _planner()
    pl = _ref["pl"]
    pl.set_params(params)
    pl.set_obstacles(obs)
    if grid is None:
        pl.set_occupancy(cells2d=None)
    else:
        pl.set_occupancy(*grid)
    pl.set_occupancy_clearance(clear_max)
    return pl


def _path_of(snap, ids, off, nr):
    raw = (abi.Node * len(ids))()
    local = np.concatenate([[0], np.cumsum(nr)])
    for i, k in enumerate(ids):
        raw[i] = snap.raw[int(k)]
        raw[i].row_offset = int(local[i])
        raw[i].nrows = int(nr[i])
    rows = np.concatenate([snap.rows[o:o + r] for o, r in zip(off, nr)])
    return raw, rows, local


def _expect(snap, root, pose, t_shift, ref):
    """What clrrt_tree_rebase(root, pose, t_shift) must leave, from the references (ref: the configured second
    planner).  Where the root's row collides (root_collides) only the counts of the subtree are filled in."""
    nd = snap.nodes
    member, _, level, _ = rebase_ref.closure(nd["parent"], root)
    mids = np.flatnonzero(member)
    off, nr = rebase_ref.node_rows(nd, mids, root)
    raw, rows, local = _path_of(snap, mids, off, nr)
    ref.path_load(raw, rows)
    ref.path_transform(False, pose)
    hraw, hrows = ref.path_download()
    hn = clrrt.nodes_to_numpy(hraw)
    rows_t = rebase_ref.shift_rows(hrows, pose, t_shift)
    dist = ref.check_obs_distance(rows_t)
    invalid = np.zeros(snap.n, dtype=bool)
    for i, k in enumerate(mids):
        invalid[k] = bool((dist[local[i]:local[i + 1]] == 0).any())
    e = dict(nodes_before=snap.n, rows_before=len(snap.rows), nodes_subtree=int(member.sum()),
             nodes_collided=int((invalid & member).sum() - invalid[root]), root_collides=bool(invalid[root]),
             invalid=invalid, member=member)
    if invalid[root]:
        return e
    _, kept, _, _ = rebase_ref.closure(nd["parent"], root, invalid)
    ids, par = rebase_ref.renumber(kept, nd["parent"], root)
    sel = np.searchsorted(mids, ids)  # kept nodes as indices into the member path
    state = hn["state"][sel].copy()
    state[:, 6] = state[:, 6] - np.float64(t_shift)
    nrows = nr[sel]
    e.update(kept=kept, ids=ids, parent=par, state=state, ref_front=hn["ref_front"][sel], ref_back=hn["ref_back"][sel],
             ang_par=hn["ang_par"][sel], ref_vback=nd["ref_vback"][ids], costE=rebase_ref.cost_e(nd["costE"], root)[ids],
             nrows=nrows.astype(np.int32), row_offset=np.concatenate([[0], np.cumsum(nrows)[:-1]]).astype(np.int64),
             rows=np.concatenate([rows_t[local[i]:local[i + 1]] for i in sel]),
             nodes_kept=len(ids), rows_kept=int(nrows.sum()), depth=int(level[kept].max()) + 1)
    return e


def _check(pl, info, e, label=""):
    assert info["outcome"] == abi.REBASE_KEPT, (label, info)
    for k in ("nodes_before", "rows_before", "nodes_subtree", "nodes_collided", "nodes_kept", "rows_kept", "depth"):
        assert info[k] == e[k], (label, k, info[k], e[k])
    assert pl.size() == (e["nodes_kept"], e["rows_kept"]), label
    g = pl.nodes()
    for k in ("parent", "nrows", "row_offset"):
        assert np.array_equal(g[k], e[k]), (label, k, np.flatnonzero(g[k] != e[k])[:8])
    for k in ("state", "ref_front", "ref_back", "ang_par", "ref_vback", "costE"):
        assert np.array_equal(_bits(g[k]), _bits(e[k])), (label, k)
    assert not g["owner"].any(), label
    assert np.array_equal(_bits(pl.rows(0, e["rows_kept"])), _bits(e["rows"])), label


def _descendants(parent):
    """Descendant counts (parents precede children)."""
    cnt = np.zeros(len(parent), dtype=np.int64)
    for k in range(len(parent) - 1, 0, -1):
        cnt[parent[k]] += cnt[k] + 1
    return cnt


def _depth(parent):
    d = np.zeros(len(parent), dtype=np.int64)
    for k in range(1, len(parent)):
        d[k] = d[parent[k]] + 1
    return d


def _pick_root(nd, min_desc=20, depths=(1, 2)):
    cnt, d = _descendants(nd["parent"]), _depth(nd["parent"])
    ok = np.flatnonzero((cnt >= min_desc) & np.isin(d, depths))
    assert len(ok), "no depth-1 / depth-2 node with enough descendants"
    return int(ok[np.argmax(cnt[ok])])


def _box_on(row, size=1.0, along=0.0, side=0.0):
    """A box obstacle on the vehicle box (4.848 m x 2 m about a centre 1.424 m ahead of the state) of a (transformed)
    row: at its centre, or `along` / `side` metres from it along / across the heading."""
    c, s = np.cos(row[2]), np.sin(row[2])
    return [row[0] + (1.424 + along) * c - side * s, row[1] + (1.424 + along) * s + side * c, 0.0, size, size, 0.0, 0.0]


# Where on a row's vehicle box the tests try their box: the trees here start at rest, so a node's middle row lies
# within a vehicle length of the state its siblings (and its parent's last row) start from, and a box at the centre
# usually takes them too; one at the nose or a front corner more often spares them.  The reference decides.
PLACES = [dict(size=1.0), dict(size=0.3, along=2.3), dict(size=0.3, along=2.3, side=0.9),
          dict(size=0.3, along=2.3, side=-0.9)]


# ---------------------------------------------------------------------------------- 1. subtree and transform
def test_subtree_and_transform():
    pl = _planner()
    try:
        _grow(pl)
        snap = Snap(pl)
        root = _pick_root(snap.nodes)
        t_shift = float(snap.nodes["state"][root, 6])
        obs = _scene_in(POSE)
        e = _expect(snap, root, POSE, t_shift, _ref_planner(pl.params, obs))
        assert not e["root_collides"] and e["nodes_subtree"] >= 21
        pl.set_obstacles(obs)
        c0 = pl.counters()
        info = pl.tree_rebase(root, POSE, t_shift)
        print(f"root {root}: {info}")
        _check(pl, info, e)
        assert pl.counters() == c0
        g = pl.nodes()
        assert g["parent"][0] == -1 and g["nrows"][0] == 1 and g["costE"][0] == 0.0
    finally:
        pl.close()


# ---------------------------------------------------------------------------------- 2. revalidation
@pytest.mark.parametrize("mode", ["box", "cell"])
def test_revalidation(mode):
    pl = _planner()
    try:
        _grow(pl)
        snap = Snap(pl)
        nd = snap.nodes
        root = _pick_root(nd)
        t_shift = float(nd["state"][root, 6])
        obs = _scene_in(POSE)
        base = _expect(snap, root, POSE, t_shift, _ref_planner(pl.params, obs))
        # an interior kept node with a kept sibling: the box goes on its middle row
        par, kept = nd["parent"], base["kept"]
        cnt = _descendants(par)
        cands = [k for k in np.flatnonzero(kept) if k != root and cnt[k] >= 1 and 3 <= nd["nrows"][k] and
                 any(kept[s] and s != k for s in np.flatnonzero(par == par[k]))]
        assert cands, "no interior node with a sibling"
        # siblings leave the same state, so a box on one often takes the others: the longest candidates first, and the
        # first whose box (by the reference) spares the root and one of its siblings
        params = pl.params if mode == "box" else clrrt.default_params(collision_mode=OCC)
        tries = [(int(k), pc) for k in sorted(cands, key=lambda k: -nd["nrows"][k])[:12] for pc in PLACES]
        for victim, place in tries:
            vi = int(np.flatnonzero(base["ids"] == victim)[0])
            mid = base["rows"][base["row_offset"][vi] + base["nrows"][vi] // 2]
            bx, grid, obs = _box_on(mid, **place), None, _scene_in(POSE)
            if mode == "box":
                obs = _scene_in(POSE, bx)
            else:  # one occupied cell of a 9 x 9 grid there (inflate 0.1), collision mode 2
                cells = np.zeros((9, 9), dtype=np.uint8)
                cells[4, 4] = 1
                grid = (bx[0] - 2.25, bx[1] - 2.25, 0.5, cells, 0.1)
            e = _expect(snap, root, POSE, t_shift, _ref_planner(params, obs, grid))
            if (not e["root_collides"] and e["invalid"][victim] and
                    any(not e["invalid"][s] for s in np.flatnonzero(par == par[victim]))):
                break
        assert not e["root_collides"] and e["invalid"][victim]
        if mode == "cell":
            pl.set_params(params)
            pl.set_occupancy(*grid)
        pl.set_obstacles(obs)
        info = pl.tree_rebase(root, POSE, t_shift)
        print(f"{mode}: victim {victim} ({cnt[victim]} descendants): {info}")
        _check(pl, info, e, mode)
        # the victim and its descendants are gone, kept siblings stay
        sub, _, _, _ = rebase_ref.closure(par, victim)
        assert not e["kept"][sub].any() and not np.isin(np.flatnonzero(sub), e["ids"]).any()
        sib = [s for s in np.flatnonzero(par == par[victim]) if s != victim and not e["invalid"][s]]
        assert sib and all(s in e["ids"] for s in sib)
        assert info["nodes_collided"] == e["nodes_collided"] >= 1
        assert info["nodes_kept"] < base["nodes_kept"]
    finally:
        pl.close()


# ---------------------------------------------------------------------------------- 3. root collision
def test_root_collision_leaves_everything_as_it_was():
    pl = _planner()
    try:
        _grow(pl)
        snap = Snap(pl)
        root = _pick_root(snap.nodes)
        t_shift = float(snap.nodes["state"][root, 6])
        base = _expect(snap, root, POSE, t_shift, _ref_planner(pl.params, _scene_in(POSE)))
        obs = _scene_in(POSE, _box_on(base["rows"][0]))
        e = _expect(snap, root, POSE, t_shift, _ref_planner(pl.params, obs))
        assert e["root_collides"]
        pl.set_obstacles(obs)
        c0, s0 = pl.counters(), pl.size()
        info = pl.tree_rebase(root, POSE, t_shift)
        assert info["outcome"] == abi.REBASE_ROOT_COLLIDES, info
        assert info["nodes_before"] == snap.n and info["nodes_subtree"] == e["nodes_subtree"]
        assert pl.size() == s0 and pl.counters() == c0
        assert Snap(pl).same_as(snap)
    finally:
        pl.close()


# ---------------------------------------------------------------------------------- 4. chain costs
def _cost_setup(kind):
    """(params, occupancy grid or None, clear_max) of a chain-cost run."""
    if kind == "default":
        return clrrt.default_params(collision_mode=OBB), None, 0.0
    p = clrrt.default_params(collision_mode=OCC if kind == "clearance" else OBB)
    p.Wcost[2] = 1.0
    if kind == "w2":
        return p, None, 0.0
    cells = np.zeros((64, 96), dtype=np.uint8)
    cells[6, 10:80] = 1  # a wall along y = -12.75, beside the corridor the tree grows in
    return p, (-4.0, -16.0, 0.5, cells), 6.0


@pytest.mark.parametrize("kind", ["default", "w2", "clearance"])
def test_chain_costs_equal_reinit(kind):
    params, grid, clear_max = _cost_setup(kind)
    pl = _planner()
    try:
        _grow(pl)
        snap = Snap(pl)
        nd = snap.nodes
        root = _pick_root(nd, depths=(1,))
        # the new car stands half a metre behind the root node, heading as it does: its subtree lies ahead
        x, y, th = nd["state"][root, :3]
        pose = (x - 0.5 * np.cos(th), y - 0.5 * np.sin(th), th)
        t_shift = float(nd["state"][root, 6])
        obs = _scene_in(pose)
        pl.set_params(params)
        pl.set_obstacles(obs)
        if grid is not None:
            pl.set_occupancy(*grid)
        pl.set_occupancy_clearance(clear_max)
        ref = _ref_planner(params, obs, grid, clear_max)
        e = _expect(snap, root, pose, t_shift, ref)
        info = pl.tree_rebase(root, pose, t_shift)
        _check(pl, info, e, kind)
        after = Snap(pl)
        g = after.nodes
        leaves = np.setdiff1d(np.arange(after.n), g["parent"])
        picks = leaves[np.unique(np.linspace(0, len(leaves) - 1, 32).astype(int))]
        last_x = after.rows[g["row_offset"] + g["nrows"] - 1, 0]
        done, seen = 0, set()
        for leaf in picks:
            chain = [int(leaf)]
            while g["parent"][chain[-1]] >= 0:
                chain.append(int(g["parent"][chain[-1]]))
            chain = chain[::-1]
            if (last_x[chain] < 0).any():
                continue
            done += 1
            raw, rows, _ = _path_of(after, chain, g["row_offset"][chain], g["nrows"][chain])
            ref.path_load(raw, rows)
            oc = ref.tree_init_from_path([0.0, 0.0, 0.0, 0.0, g["state"][0, 4], 0.0])
            assert oc == abi.REINIT_KEPT, (kind, leaf, oc)
            r = ref.nodes()
            assert len(r["costS"]) == len(chain)
            assert np.array_equal(_bits(r["costS"]), _bits(g["costS"][chain])), (kind, leaf)
            assert np.array_equal(r["goal"], g["goal"][chain]), (kind, leaf)
            seen.update(chain)
        print(f"{kind}: {done} of {len(picks)} sampled chains qualify, {len(seen)} nodes checked, "
              f"{int(g['goal'].sum())} goal nodes, costS range {g['costS'].min()} .. {g['costS'].max()}")
        assert done >= 8, (done, len(picks))
        if kind == "clearance":  # the field is baked, so the rebase and re-init both took the clearance
            assert pl.occupancy_clearance_info()["baked"]
    finally:
        pl.close()


# ---------------------------------------------------------------------------------- 5. sizes
@pytest.mark.parametrize("size", [1, 2, 63, 64, 65])
def test_subtree_sizes(size):
    pl = _planner()
    try:
        _grow(pl)
        full = Snap(pl)
        par = full.nodes["parent"]
        if size == 1:
            root, n = full.n - 1, full.n  # the last node is a leaf
        else:  # a root with more descendants than needed, the tree truncated where its subtree has `size` nodes: the
            # inner node with the most descendants where that is enough, else node 0 (a four-round tree is bushy at
            # its root: its largest inner subtree has some 50 nodes)
            cnt = _descendants(par)
            root = int(np.argmax(cnt[1:])) + 1
            if cnt[root] < size:
                root = 0
            members = np.flatnonzero(rebase_ref.closure(par, root)[0])
            n = int(members[size])
            pl.tree_truncate(n)
        snap = Snap(pl, n)
        snap.rows = full.rows[:pl.size()[1]]
        t_shift = float(snap.nodes["state"][root, 6])
        obs = _scene_in(POSE)
        e = _expect(snap, root, POSE, t_shift, _ref_planner(pl.params, obs))
        assert e["nodes_subtree"] == size and not e["root_collides"]
        pl.set_obstacles(obs)
        info = pl.tree_rebase(root, POSE, t_shift)
        _check(pl, info, e, f"size {size}")
        if size == 1:
            assert info["nodes_kept"] == 1 and info["rows_kept"] == 1 and info["depth"] == 1
    finally:
        pl.close()


def _chain_path(n, nrows=3):
    """A straight committed path of n nodes driving along +x at 1 m/s."""
    raw = (abi.Node * n)()
    rows = np.zeros((n * nrows, 10))
    for i in range(n):
        for r in range(nrows):
            q = i * nrows + r
            rows[q, 0] = 0.25 * (q + 1)
            rows[q, 4] = 1.0
            rows[q, 6] = 0.25 * (q + 1)
        nd = raw[i]
        for k in range(10):
            nd.state[k] = rows[i * nrows + nrows - 1, k]
        nd.ref_front[0], nd.ref_back[0] = 0.25 * i * nrows, 0.25 * (i + 1) * nrows
        nd.ref_vback, nd.ang_par, nd.parent = 1.0, 0.0, i - 1
        nd.costE = 0.25 * (i + 1) * nrows
        nd.nrows, nd.row_offset = nrows, i * nrows
    return raw, rows


def test_chain_of_70_rebased_at_node_3():
    params = clrrt.default_params(collision_mode=STUB)
    pl = _planner(params)
    try:
        raw, rows = _chain_path(70)
        pl.path_load(raw, rows)
        assert pl.tree_init_from_path([0.0, 0.0, 0.0, 0.0, 1.0, 0.0]) == abi.REINIT_KEPT
        assert pl.size() == (70, 210)
        snap = Snap(pl)
        pose = (float(snap.nodes["state"][3, 0]) - 0.1, 0.05, 0.01)
        t_shift = float(snap.nodes["state"][3, 6])
        e = _expect(snap, 3, pose, t_shift, _ref_planner(params, np.zeros((0, 7))))
        info = pl.tree_rebase(3, pose, t_shift)
        _check(pl, info, e, "chain")
        assert info["depth"] == 67 and info["nodes_kept"] == 67 and info["rows_kept"] == 1 + 66 * 3
        assert np.array_equal(pl.nodes()["parent"], np.arange(-1, 66))
    finally:
        pl.close()


# ---------------------------------------------------------------------------------- 6. windowed move
def test_small_window_equals_the_default():
    snaps, infos = [], []
    for window in (None, 64):
        pl = _planner()
        try:
            _grow(pl)
            snap = Snap(pl)
            nd = snap.nodes
            pose = (0.4, -0.2, 0.05)
            base = _expect(snap, 0, pose, 0.0, _ref_planner(pl.params, _scene_in(pose)))
            # drop a few early nodes: a box on the middle row of an early kept node with one to five descendants
            cnt = _descendants(nd["parent"])
            early = [k for k in base["ids"][1:200] if 1 <= cnt[k] <= 5 and nd["nrows"][k] >= 3]
            assert early
            # the first box (by the reference) that spares the root and most of the tree
            for k, place in [(k, pc) for k in early[:20] for pc in PLACES]:
                vi = int(np.flatnonzero(base["ids"] == k)[0])
                mid = base["rows"][base["row_offset"][vi] + base["nrows"][vi] // 2]
                obs = _scene_in(pose, _box_on(mid, **place))
                e = _expect(snap, 0, pose, 0.0, _ref_planner(pl.params, obs))
                if not e["root_collides"] and snap.n > e["nodes_kept"] > 0.5 * snap.n:
                    break
            assert not e["root_collides"] and 1 <= snap.n - e["nodes_kept"] and e["nodes_kept"] > 0.5 * snap.n
            assert e["rows_kept"] > 64 * 8  # many windows, destinations overlapping earlier sources
            pl.set_obstacles(obs)
            if window:
                pl.set_option("rebase_window_rows", window)
            info = pl.tree_rebase(0, pose, 0.0)
            _check(pl, info, e, f"window {window}")
            snaps.append(Snap(pl))
            infos.append({k: v for k, v in info.items() if k != "device_ms"})
        finally:
            pl.close()
    assert infos[0] == infos[1] and snaps[0].same_as(snaps[1])


# ---------------------------------------------------------------------------------- 7. growing on
def _rebased(strategy=None, defer=0):
    pl = _planner()
    _grow(pl)
    nd = pl.nodes()
    root = _pick_root(nd, depths=(1,))
    x, y, th = nd["state"][root, :3]
    pose = (x - 0.5 * np.cos(th), y - 0.5 * np.sin(th), th)
    pl.set_params(clrrt.default_params(goal=replan.goal_in_car_frame((40.0, 0.0, 0.0, 0.0), pose), collision_mode=OBB))
    pl.set_obstacles(_scene_in(pose))
    info = pl.tree_rebase(root, pose, float(nd["state"][root, 6]))
    assert info["outcome"] == abi.REBASE_KEPT and info["nodes_kept"] >= 21
    return pl, pose


def _grow_on(pl, strategy, defer):
    if strategy:
        nn_strategy(pl, strategy)
    pl.set_option("defer_steps", defer)
    return pl.expand(clrrt.Rng(99), n_iters=B * 3, mode=clrrt.CLRRT_MODE_BATCH, batch=B)


@pytest.mark.parametrize("defer", [0, 32])
def test_growing_on_after_a_rebase(defer):
    runs = {}
    try:
        for strategy in ("brute", "walk", "walk_split"):
            pl, pose = _rebased()
            nk = pl.size()[0]
            if "loaded" not in runs:  # a fresh context that loads the rebased headers and runs the same samples
                fresh = _planner(pl.params)
                fresh.set_obstacles(_scene_in(pose))
                fresh.tree_load(pl.nodes_raw())
                _grow_on(fresh, None, defer)
                runs["loaded"] = fresh
            st = _grow_on(pl, strategy, defer)
            assert st["rounds"] == 3 and pl.size()[0] > nk
            runs[strategy] = pl
        want = runs["brute"].nodes()
        for name, pl in runs.items():
            got = pl.nodes()
            for k in want:
                if k != "row_offset":
                    assert np.array_equal(_bits(got[k]), _bits(want[k])), (defer, name, k)
            if name != "loaded":  # (the fresh context's counters start at the load)
                assert pl.counters() == runs["brute"].counters(), (defer, name)
        rows = runs["brute"].rows(0, runs["brute"].size()[1])
        for name in ("walk", "walk_split"):
            assert np.array_equal(want["row_offset"], runs[name].nodes()["row_offset"])
            assert np.array_equal(_bits(runs[name].rows(0, runs[name].size()[1])), _bits(rows)), (defer, name)
        pl = runs["walk"]
        ids, cost, n_goal = pl.extract_best_path()
        print(f"defer {defer}: {pl.size()} nodes / rows, {n_goal} goal nodes, best path {len(ids)} nodes, cost {cost}")
        assert len(ids) >= 2 and ids[0] == 0
        assert pl.path_commit(ids) == 0
        praw, prows = pl.path_download()
        tree_rows = np.concatenate([rows[want["row_offset"][i]:want["row_offset"][i] + want["nrows"][i]] for i in ids])
        assert np.array_equal(_bits(prows), _bits(tree_rows))
    finally:
        for pl in runs.values():
            pl.close()


# ---------------------------------------------------------------------------------- 8. errors
def test_errors():
    import torch

    pl = _planner()
    try:
        _grow(pl, rounds=1)
        n = pl.size()[0]
        before = Snap(pl)
        for bad in (-1, n, n + 5):
            with pytest.raises(clrrt.ClrrtError, match=r"-> -1"):
                pl.tree_rebase(bad, POSE, 0.0)
        for pose, ts in (((np.nan, 0.0, 0.0), 0.0), ((0.0, np.inf, 0.0), 0.0), ((0.0, 0.0, np.nan), 0.0),
                         ((0.0, 0.0, 0.0), np.nan)):
            with pytest.raises(clrrt.ClrrtError, match=r"-> -1"):
                pl.tree_rebase(0, pose, ts)
        buf = torch.empty(64 * C.sizeof(abi.Node), dtype=torch.uint8, device="cuda")
        hook = clrrt.EXCHANGE_FN(lambda user, io: 0)
        pl.set_shards(0, 2, buf.data_ptr(), 64, hook)
        with pytest.raises(clrrt.ClrrtError, match=r"-> -4"):
            pl.tree_rebase(0, POSE, 0.0)
        pl.set_shards(0, 1)
        assert Snap(pl).same_as(before)
        raw = pl.nodes_raw()
        pl.tree_load(raw)
        with pytest.raises(clrrt.ClrrtError, match=r"-> -4"):
            pl.tree_rebase(0, POSE, 0.0)
        pl.expand(clrrt.Rng(5), n_iters=B, mode=clrrt.CLRRT_MODE_BATCH, batch=B)  # still rowless at its base
        with pytest.raises(clrrt.ClrrtError, match=r"-> -4"):
            pl.tree_rebase(0, POSE, 0.0)
    finally:
        pl.close()
