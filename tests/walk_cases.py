"""One adversarial tree and its samples for the walk index tests (tests/test_walk_index.py).  No tests here.

The tree is made of records in numpy and loaded with tree_load; every position, ref.back() point and sample lies
inside the default sample region (goal (40, 0): x in [-2, 52], y in [-9, 9]), so nn_setup's frame assumption holds.

Main tree, N = 2 * 1024 + 13 * 32 + 7 = 2471 nodes (three super-tiles, the last partial, the last tile partial), ids
shuffled (node 0 stays the root):
  * scattered nodes, random headings, costE from 25 shared values in [0, 200];
  * four clusters of 96 nodes and one of 32 with small discs and heading arcs (three tiles' worth each, so whole
    tiles with small bounds lie inside them);
  * the root class: node 0 and 1099 copies of its key inputs (x, y, heading, costE) with distinct ref.back() points on
    a ring and scattered ids -- longer than a super-tile and than the roster's 64;
  * a non-root run: 40 records with another pose's key inputs;
  * 32 headings straddling +-pi, 32 spread over the full circle, and the same two groups for ang_par (the groups'
    position puts them in few tiles, so tiles and super-tiles with heading arcs past the "unbounded" limit exist;
    the place order starts with the ang_par sector, so no tile of this tree spans the ang_par circle: the small
    trees' single tiles do);
  * three non-finite records: NaN x, +inf costE, NaN ref.back() (clrrt_tree_load takes them: they enter no list and
    their tiles carry no bound).  finite_for_oracle() gives the same tree with the NaN-x record's x made finite and
    its ref.back() NaN instead: a NaN key has no place in the oracle's std::stable_sort order, and either record is
    in no list.
Far frame (index checks only): far_tree(), the frame of a goal 2 km away.
Small trees (index checks only): small_tree(n); n = 32 holds headings and ang_par balanced over the circle, the tile
whose arcs have no mean direction.

256 samples, half of every group explore and half optimize: see samples().
"""
import numpy as np

from clrrt import abi

RHO = 4.77
REGION = (-2.0, -9.0, 52.0, 9.0)
N_MAIN = 2 * 1024 + 13 * 32 + 7
SMALL_SIZES = (1, 31, 32, 33, 1023, 1024, 1025)
CLUSTER_SIZES = (96, 96, 96, 96, 32)  # three tiles' worth: at least two whole tiles lie inside a cluster's records
N_CLUSTERS = len(CLUSTER_SIZES)
ROOT_COPIES = 1099
RUN_LEN = 40
ROOT_HEADING = 0.9  # the far side of the root's right turning circle lies inside the region

FIELDS = ("x", "y", "h", "ce", "bx", "by", "fx", "fy", "ap")


def _records(n):
    return {k: np.zeros(n, dtype=np.float32 if k == "ce" else np.float64) for k in FIELDS}


def _finish(r):
    """ang_par as the engine and the reference form it: atan2(ref.back() - ref.front())."""
    r["ap"] = np.arctan2(r["by"] - r["fy"], r["bx"] - r["fx"])
    return r


def _set_refs(r, sl, bx, by, ap):
    r["bx"][sl], r["by"][sl] = bx, by
    r["fx"][sl], r["fy"][sl] = bx - np.cos(ap), by - np.sin(ap)


def _scattered(rng, r, sl, n, ap_hi=1.5):
    costs = np.round(rng.uniform(0.0, 200.0, 25), 2).astype(np.float32)
    r["x"][sl], r["y"][sl] = rng.uniform(0.0, 50.0, n), rng.uniform(-7.0, 7.0, n)
    r["h"][sl] = rng.uniform(-np.pi, np.pi, n)
    r["ce"][sl] = costs[rng.integers(0, 25, n)]
    a, d = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.0, 1.0, n)
    _set_refs(r, sl, r["x"][sl] + d * np.cos(a), r["y"][sl] + d * np.sin(a), rng.uniform(-np.pi, ap_hi, n))


def cluster_params():
    """Centres, mean headings (along the road, either way), nominal disc radii and heading half-arcs."""
    rng = np.random.default_rng(77)
    cx, cy = rng.uniform(8.0, 42.0, N_CLUSTERS), rng.uniform(-5.0, 5.0, N_CLUSTERS)
    hd = rng.uniform(-0.5, 0.5, N_CLUSTERS) + np.pi * rng.integers(0, 2, N_CLUSTERS)
    hd = (hd + np.pi) % (2 * np.pi) - np.pi
    pr = rng.uniform(0.02, 0.3, N_CLUSTERS)
    th = np.deg2rad(rng.uniform(0.5, 6.0, N_CLUSTERS))
    return cx, cy, hd, pr, th


def abeam_normal(c):
    """The unit normal of cluster c's mean heading on the side of y = 0 (where its abeam samples lie)."""
    cx, cy, hd, _, _ = cluster_params()
    nx, ny = -np.sin(hd[c]), np.cos(hd[c])
    return (-nx, -ny) if cy[c] * ny > 0 else (nx, ny)


def main_records():
    """The main tree's records in generation order (dict of arrays) and the groups' index ranges."""
    rng = np.random.default_rng(2471)
    n = N_MAIN
    r = _records(n)
    groups = {}
    k = 0

    def take(name, m):
        nonlocal k
        groups[name] = slice(k, k + m)
        k += m
        return groups[name]

    # the root and its class
    sl = take("root", 1 + ROOT_COPIES)
    r["x"][sl], r["y"][sl], r["h"][sl], r["ce"][sl] = 2.0, 0.25, ROOT_HEADING, 0.0
    phi = -np.pi + 2 * np.pi * ((np.arange(1 + ROOT_COPIES) * 0.6180339887) % 1.0)
    _set_refs(r, sl, 2.0 + 3.0 * np.cos(phi), 0.25 + 3.0 * np.sin(phi), phi)
    r["fx"][sl], r["fy"][sl] = 2.0, 0.25
    # a non-root run
    sl = take("run", RUN_LEN)
    r["x"][sl], r["y"][sl], r["h"][sl], r["ce"][sl] = 23.5, -1.75, 0.6, np.float32(31.25)
    phi = 0.3 + 0.4 * np.arange(RUN_LEN) / RUN_LEN
    _set_refs(r, sl, 23.5 + 1.5 * np.cos(phi), -1.75 + 1.5 * np.sin(phi), phi)
    # clustered tiles (the generator idea of test_walk_circle_bound._tiles / _members)
    cx, cy, hd, prn, thn = cluster_params()
    for c in range(N_CLUSTERS):
        m = CLUSTER_SIZES[c]
        sl = take(f"cluster{c}", m)
        rad = prn[c] * np.sqrt(rng.uniform(0, 1, m))
        rad[:16] = prn[c]
        a = rng.uniform(-np.pi, np.pi, m)
        dh = thn[c] * rng.uniform(-1, 1, m)
        dh[:8] = thn[c] * rng.choice([-1.0, 1.0], 8)
        r["x"][sl], r["y"][sl] = cx[c] + rad * np.cos(a), cy[c] + rad * np.sin(a)
        r["h"][sl] = hd[c] + dh
        r["ce"][sl] = (2.0 + 1.2 * np.hypot(cx[c] - 2.0, cy[c])).astype(np.float32)
        # ang_par along the heading, or (even clusters) turned to 0.4 rad off the abeam side: the samples abeam are
        # then inside the feasibleNode cone, and the tile's bound is the turning bound, not "infeasible"
        ap = hd[c] + 0.5 * dh
        if c % 2 == 0:
            ap = np.arctan2(abeam_normal(c)[1], abeam_normal(c)[0]) + 0.4 + 0.5 * dh
        _set_refs(r, sl, r["x"][sl] + 0.2 * np.cos(r["h"][sl]), r["y"][sl] + 0.2 * np.sin(r["h"][sl]), ap)
    # heading edge cases (ang_par in a sector the scattered nodes leave empty)
    for name, hs in (("h_straddle", np.pi + rng.uniform(-0.1, 0.1, 32)), ("h_circle", -np.pi + 2 * np.pi * np.arange(32) / 32)):
        sl = take(name, 32)
        c0 = (30.0, 3.0) if name == "h_straddle" else (14.0, -3.0)
        a, d = rng.uniform(-np.pi, np.pi, 32), rng.uniform(0, 0.3, 32)
        r["x"][sl], r["y"][sl] = c0[0] + d * np.cos(a), c0[1] + d * np.sin(a)
        r["h"][sl] = (hs + np.pi) % (2 * np.pi) - np.pi
        r["ce"][sl] = np.float32(40.0)
        _set_refs(r, sl, r["x"][sl], r["y"][sl], 2.0 + rng.uniform(-0.2, 0.2, 32))
    # ang_par edge cases
    for name, aps in (("ap_straddle", np.pi + rng.uniform(-0.1, 0.1, 32)), ("ap_circle", -np.pi + 2 * np.pi * np.arange(32) / 32)):
        sl = take(name, 32)
        c0 = (36.0, -4.0) if name == "ap_straddle" else (19.0, 4.0)
        a, d = rng.uniform(-np.pi, np.pi, 32), rng.uniform(0, 0.3, 32)
        r["x"][sl], r["y"][sl] = c0[0] + d * np.cos(a), c0[1] + d * np.sin(a)
        r["h"][sl] = 0.3 + rng.uniform(-0.05, 0.05, 32)
        r["ce"][sl] = np.float32(55.5)
        _set_refs(r, sl, r["x"][sl], r["y"][sl], (aps + np.pi) % (2 * np.pi) - np.pi)
    # non-finite records
    sl = take("nonfinite", 3)
    _scattered(rng, r, sl, 3)
    # scattered nodes
    sl = take("scattered", n - k)
    _scattered(rng, r, sl, sl.stop - sl.start)
    assert k == n
    nf = groups["nonfinite"].start
    r["x"][nf] = np.nan
    r["ce"][nf + 1] = np.inf
    r["bx"][nf + 2] = np.nan
    return _finish(r), groups


def main_tree():
    """(records by node id, groups as id arrays): the generation order shuffled, node 0 the root."""
    r, groups = main_records()
    perm = np.concatenate([[0], 1 + np.random.default_rng(5).permutation(N_MAIN - 1)])  # id -> generation index
    inv = np.empty(N_MAIN, dtype=np.int64)
    inv[perm] = np.arange(N_MAIN)
    out = {k: v[perm] for k, v in r.items()}
    return out, {name: np.sort(inv[sl]) for name, sl in groups.items()}


def finite_for_oracle(rec, groups):
    """The tree with the NaN-x record's x finite and its ref.back() NaN (module docstring)."""
    out = {k: v.copy() for k, v in rec.items()}
    i = int(np.nonzero(np.isnan(rec["x"]))[0][0])
    out["x"][i] = 25.0
    out["bx"][i] = np.nan
    return out


def small_tree(n):
    rng = np.random.default_rng(100 + n)
    r = _records(n)
    _scattered(rng, r, slice(0, n), n, ap_hi=np.pi)
    if n == 32:  # balanced arcs: no mean direction
        a = -np.pi + 2 * np.pi * np.arange(32) / 32
        r["h"][:] = a
        _set_refs(r, slice(0, n), r["x"], r["y"], a[::-1])
    if n >= 1023:  # a run of equal records across the first super-tile's end is likely: 80 copies of one pose
        sl = slice(n // 2, n // 2 + 80)
        r["x"][sl], r["y"][sl], r["h"][sl], r["ce"][sl] = 25.0, 0.5, -2.0, np.float32(12.5)
        phi = 0.1 + 0.4 * np.arange(80) / 80  # one ang_par sector: equal records are neighbours within a sector
        _set_refs(r, sl, 25.0 + np.cos(phi), 0.5 + np.sin(phi), phi)
    return _finish(r)


FAR_GOAL = (2000.0, 0.0, 0.0, 0.0)


def far_tree():
    """1025 nodes in the sample region of a goal 2 km away (x in [-2, 2012]): frame coordinates up to 1000 m, where a
    float coordinate errs by up to 3e-5 m -- more than the discs' fixed 1e-5, so only the builder's frame slack keeps
    the exact positions inside.  Ten clusters of 96 nodes within 5 cm (whole tight tiles inside them) far from the
    frame's centre, and scattered nodes."""
    rng = np.random.default_rng(2000)
    n = 1025
    r = _records(n)
    _scattered(rng, r, slice(0, n), n)
    r["x"][:] = rng.uniform(0.0, 2000.0, n)
    _set_refs(r, slice(0, n), r["x"] + 0.3, r["y"], rng.uniform(-np.pi, 1.5, n))
    for c in range(10):
        sl = slice(1 + 96 * c, 1 + 96 * (c + 1))
        cx = rng.uniform(5.0, 300.0) if c % 2 else rng.uniform(1700.0, 1995.0)
        cy = rng.uniform(-6.0, 6.0)
        a, d = rng.uniform(-np.pi, np.pi, 96), 0.05 * np.sqrt(rng.uniform(0, 1, 96))
        r["x"][sl], r["y"][sl] = cx + d * np.cos(a), cy + d * np.sin(a)
        r["h"][sl] = 0.2 + rng.uniform(-0.02, 0.02, 96)
        r["ce"][sl] = np.float32(1.1 * cx)
        _set_refs(r, sl, r["x"][sl] + 0.2, r["y"][sl] + 0.05, 0.3 + rng.uniform(-0.02, 0.02, 96))
    return _finish(r)


def nodes_raw(rec):
    """abi.Node array of the records (parent 0, the root -1)."""
    n = rec["x"].size
    nodes = (abi.Node * n)()
    for i in range(n):
        d = nodes[i]
        d.state[0], d.state[1], d.state[2] = rec["x"][i], rec["y"][i], rec["h"][i]
        d.ref_front[0], d.ref_front[1] = rec["fx"][i], rec["fy"][i]
        d.ref_back[0], d.ref_back[1] = rec["bx"][i], rec["by"][i]
        d.ref_vback = 1.0
        d.ang_par = rec["ap"][i]
        d.costE = rec["ce"][i]
        d.parent = -1 if i == 0 else 0
    return nodes


def samples(rec, groups, feas_len):
    """(x, y, explore, group name) of the 256 samples."""
    rng = np.random.default_rng(256)
    pts = []

    def add(name, xs, ys):
        for x, y in zip(np.atleast_1d(xs), np.atleast_1d(ys)):
            pts.append((float(x), float(y), name))

    sc = groups["scattered"]
    inner = sc[(rec["x"][sc] > 12) & (rec["x"][sc] < 40) & (np.abs(rec["y"][sc]) < 1.0)]
    assert inner.size >= 8
    add("uniform", rng.uniform(-1.9, 51.9, 128), rng.uniform(-8.9, 8.9, 128))
    on = np.concatenate([sc[:5], groups["root"][:1], groups["run"][:1], groups["cluster0"][:1]])
    add("on_node", rec["x"][on], rec["y"][on])
    cl = [groups[f"cluster{c}"] for c in range(N_CLUSTERS)]
    cl = [g for g in cl[:4]] + [g[:48] for g in cl[:4]]  # (the clusters' means: inside the discs of their tiles)
    add("tile_centre", [rec["x"][g].mean() for g in cl], [rec["y"][g].mean() for g in cl])
    onb = np.concatenate([sc[5:10], groups["root"][1:3], groups["run"][1:2]])
    add("on_ref_back", rec["bx"][onb], rec["by"][onb])
    # on the turning circle of chosen records: t2 = dc^2 - rho^2 about the circle centre at rho abeam (towards y = 0)
    # the root class's tiles are the tightest of the tree (one position, one heading), so the tile bound's circle
    # floor decides next to the circle itself: samples just short of the far side of the root's right circle, 0.06 and
    # 0.03 rad of arc before the point abeam (keys rho (pi - 0.06), below the floor's 14.9 when outside the circle)
    for i in list(inner[:3]) + [0]:
        h = rec["h"][i]
        nx, ny = -np.sin(h), np.cos(h)
        if i == 0 or abs(rec["y"][i] + RHO * ny) > abs(rec["y"][i] - RHO * ny):
            nx, ny = -nx, -ny
        ccx, ccy = rec["x"][i] + RHO * nx, rec["y"][i] + RHO * ny
        back = np.arctan2(-ny, -nx)  # the direction from the circle centre to the node
        for t2 in (-0.02, -0.01, -1e-3, 0.0, 1e-3, 0.01, 0.02):
            dc = np.sqrt(RHO * RHO + t2)
            for a in ((0.6, -1.6) if i else (-(np.pi - 0.06), -(np.pi - 0.03))):
                add("circle", ccx + dc * np.cos(back + a), ccy + dc * np.sin(back + a))
    # abeam of the clustered tiles, towards y = 0
    cx, cy, hd, _, _ = cluster_params()
    for c in range(4):
        nx, ny = abeam_normal(c)
        for d in (0.5 * RHO, RHO, 2 * RHO):
            for along in (-0.3, 0.3):
                add("abeam", cx[c] + d * nx + along * np.cos(hd[c]), cy[c] + d * ny + along * np.sin(hd[c]))
    for i in inner[4:8]:
        for e in (-1e-4, 1e-4):
            add("feas_len", rec["bx"][i] + (feas_len + e) * np.cos(rec["ap"][i]),
                rec["by"][i] + (feas_len + e) * np.sin(rec["ap"][i]))
    for i in inner[:4]:
        for side in (-1.0, 1.0):
            for e in (-1e-3, 1e-3):
                a = rec["ap"][i] + side * (np.pi / 4 + e)
                add("cone_edge", rec["bx"][i] + 5.0 * np.cos(a), rec["by"][i] + 5.0 * np.sin(a))
    assert len(pts) == 256, len(pts)
    x, y = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    assert (x > REGION[0]).all() and (x < REGION[2]).all() and (y > REGION[1]).all() and (y < REGION[3]).all()
    names = np.array([p[2] for p in pts])
    explore = np.isin(np.arange(256) % 4, (0, 3)).astype(np.int32)  # half of every group, either flag at every case kind
    return x, y, explore, names


def sample_structs(x, y, explore):
    return [abi.Sample(float(a), float(b), int(e), 0) for a, b, e in zip(x, y, explore)]
