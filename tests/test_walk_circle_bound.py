"""The circle floor of the walk search's tile bound (walk_lb, cl-rrt_amd/csrc/clrrt_nnwalk.hip).

A tile (32 records: a disc of positions around its centre, an arc of headings around its mean heading) whose every
record surely has the sample inside a turning circle gets the key bound 14.9 -- the floor walk_key_range gives such a
record (t2 = tx^2 + ty (ty - 2 rho) <= -0.01: key >= rho pi).  The tile test: with D the centre distance, ang the
angle between the mean heading and the direction to the sample, A = asin(pr / D) + thh + 3e-3 and z = min(ang,
pi - ang) - A > 0, every record has sin(bearing) >= sin(z) and distance d in [D - pr, D + pr], so t2 <= U = max over
both ends of d (d - 2 rho sin z); the tile fires when U <= -0.011.

CPU: the test restated in float32 numpy against the float key (dubins_key_f32, walk_key_range: restated from
tests/test_nnwalk_bounds.py) of member records on the disc's rim and at the arc's ends.
GPU: a clustered synthetic tree (whole tiles with small discs and arcs) with samples abeam of the clusters, on the
circle boundary, ahead and behind: the walk's lists equal the brute force's, and pipelined rounds grow the tree of
unpipelined brute-force rounds.

The CPU part checks the formula as restated here, not the compiled kernel: walk_lb itself, given the tile records the
index builders make, is checked on the device against the exact keys of every tile member by tests/test_walk_index.py
(clrrt_selftest_walk, clrrt_debug_walk_index).
"""
import numpy as np
import pytest

F = np.float32
RHO = F(4.77)
PI = F(3.14159265)
SLACK = 2e-5  # the float frame's coordinate error of a 300 m frame (2^-24 of the coordinate bound)


# ---------------------------------------------------------------------------------------------------------------
# restated from tests/test_nnwalk_bounds.py
def dubins_key_f32(tx, ty):
    """dubinsDistance after the rotation into the node frame (ty folded to >= 0), float32 like the reference's
    float locals."""
    tx = tx.astype(F)
    ty = np.abs(ty).astype(F)
    rho = RHO
    dc = np.sqrt(tx * tx + (ty - rho) * (ty - rho))
    thc = np.arctan2(tx, rho - ty).astype(F)
    thc = np.where(thc < 0, (thc.astype(np.float64) + 2 * np.pi).astype(F), thc)
    df = np.sqrt(tx * tx + (ty + rho) * (ty + rho))
    inside = (tx * tx + (ty + rho) * (ty + rho) <= rho * rho) | (tx * tx + (ty - rho) * (ty - rho) <= rho * rho)
    with np.errstate(all="ignore"):
        out = np.sqrt(dc * dc - rho * rho) + rho * (thc - np.arccos(rho / dc))
        al = (2 * np.pi - np.arccos((5 * rho * rho - df * df) / (4 * rho * rho)).astype(np.float64)).astype(F)
        inn = rho * (al + np.arcsin(tx / df) - np.arcsin(rho * np.sin(al) / df))
    return np.where(inside, inn, out).astype(np.float64)


def key_range_lo(tx, ty):
    """walk_key_range's lower bound where it is the inside floor (t2 <= -0.01 -> 14.9); t2 as it forms it."""
    tx, ty = tx.astype(F), ty.astype(F)
    t2 = tx * tx + ty * (ty - F(2) * RHO)
    return t2, np.where(t2 <= F(-0.01), 14.9, -np.inf)


def acos_apx(x):
    x = x.astype(F)
    ax = np.minimum(np.abs(x), F(1))
    r = np.sqrt(F(1) - ax) * (F(1.5707288) + ax * (F(-0.2121144) + ax * (F(0.0742610) + ax * F(-0.0187293))))
    return np.where(x < 0, PI - r, r).astype(F)


# ---------------------------------------------------------------------------------------------------------------
def circle_floor(dx, dy, thx, thy, pr, thh):
    """walk_lb's circle test in float32: True where the tile's key bound becomes max(lb, 14.9).  (dx, dy) = sample -
    tile centre, (thx, thy) the mean heading, pr / thh the tile's (inflated) disc radius and heading half-arc."""
    dx, dy, thx, thy, pr, thh = (np.asarray(v, dtype=F) for v in (dx, dy, thx, thy, pr, thh))
    D = np.sqrt(dx * dx + dy * dy)
    with np.errstate(all="ignore"):
        iD = F(1) / D
        A = (F(1.57079633) - acos_apx(pr * iD)) + thh + F(3e-3)
        ang = acos_apx((dx * thx + dy * thy) * iD)
        z = np.minimum(ang, PI - ang) - A
        z2 = z * z
        g = (F(2) * RHO) * (z + z * z2 * (F(-1) / F(6) + z2 * (F(1) / F(120) - z2 * (F(1) / F(5040)))))
        d0, d1 = D - pr, D + pr
        U = np.maximum(d0 * (d0 - g), d1 * (d1 - g))
        return (D > pr) & (thh < F(3)) & (z > 0) & (U <= F(-0.011))


def _tiles(rng, n, abeam_share):
    """n random tiles around random frame points: nominal disc radius 0-3 m, heading half-arc 0-40 degrees, the sample
    at 0.3-12 m from the centre at any bearing; abeam_share of them drawn where the floor can apply at all (bearing
    within 45 degrees of abeam, the sample closer than the turning circle's diameter, small discs and arcs)."""
    ab = rng.uniform(0, 1, n) < abeam_share
    D = np.where(ab, rng.uniform(0.3, 8.0, n), rng.uniform(0.3, 12.0, n))
    prn = np.where(ab, rng.uniform(0, 0.6, n) * np.minimum(D, 1.0), rng.uniform(0, 3.0, n))
    thn = np.deg2rad(np.where(ab, rng.uniform(0, 12.0, n), rng.uniform(0, 40.0, n)))
    brg = np.where(ab, rng.choice([-1.0, 1.0], n) * np.deg2rad(rng.uniform(45, 135, n)), rng.uniform(-np.pi, np.pi, n))
    hd = rng.uniform(-np.pi, np.pi, n)  # the mean heading
    cx, cy = rng.uniform(-150, 150, n), rng.uniform(-150, 150, n)
    sx, sy = cx + D * np.cos(hd + brg), cy + D * np.sin(hd + brg)
    return cx, cy, hd, prn, thn, sx, sy


def _members(rng, cx, cy, hd, prn, thn, m=32):
    """m member records per tile inside the nominal disc and arc: the first 8 on the disc's rim with headings at
    the arc's ends, the next 8 on the rim, 4 at the arc's ends, the rest anywhere inside; positions jittered by the
    frame slack."""
    n = cx.size
    r = prn[:, None] * np.sqrt(rng.uniform(0, 1, (n, m)))
    r[:, :16] = prn[:, None]
    a = rng.uniform(-np.pi, np.pi, (n, m))
    dh = thn[:, None] * rng.uniform(-1, 1, (n, m))
    ends = rng.choice([-1.0, 1.0], (n, m)) * thn[:, None]
    dh[:, :8] = ends[:, :8]
    dh[:, 16:20] = ends[:, 16:20]
    ja, jr = rng.uniform(-np.pi, np.pi, (n, m)), SLACK * rng.uniform(0, 1, (n, m))
    px = cx[:, None] + r * np.cos(a) + jr * np.cos(ja)
    py = cy[:, None] + r * np.sin(a) + jr * np.sin(ja)
    return px, py, hd[:, None] + dh


def _node_frame(px, py, ph, sx, sy):
    """(tx, ty) as dubins_key forms them: the float offset rotated by the record's float (cos, sin)(-heading)."""
    qx, qy = (sx - px).astype(F), (sy - py).astype(F)
    c, s = np.cos(-ph).astype(F), np.sin(-ph).astype(F)
    return c * qx - s * qy, np.abs(s * qx + c * qy)


def _fire(cx, cy, hd, prn, thn, sx, sy, rng=None):
    """The tile test on the tile's float frame values: centre and sample rounded to float32 frame coordinates (each
    off by up to the frame slack), pr and thh inflated as walk_tile_bounds inflates them."""
    pr = prn * (1 + 1e-5) + 2 * SLACK + 1e-5
    thh = thn + 2e-3
    fx = lambda v: np.asarray(v, dtype=np.float64).astype(F)  # noqa: E731
    dx, dy = fx(sx) - fx(cx), fx(sy) - fx(cy)
    return circle_floor(dx, dy, fx(np.cos(hd)), fx(np.sin(hd)), pr, thh)


@pytest.mark.parametrize("abeam_share", [0.0, 0.35])
def test_fired_tiles_hold_only_inside_circle_records(abeam_share):
    rng = np.random.default_rng(41)
    n = 200_000
    cx, cy, hd, prn, thn, sx, sy = _tiles(rng, n, abeam_share)
    fire = _fire(cx, cy, hd, prn, thn, sx, sy)
    share = fire.mean()
    print(f"tiles fired: {fire.sum()} of {n} ({share:.3f})")
    assert share >= 1 / 20  # a condition on the generator: the term triggers
    px, py, ph = _members(rng, cx[fire], cy[fire], hd[fire], prn[fire], thn[fire])
    tx, ty = _node_frame(px, py, ph, sx[fire][:, None], sy[fire][:, None])
    t2, lo = key_range_lo(tx, ty)
    key = dubins_key_f32(tx, ty)
    print(f"fired tiles' members: max t2 {t2.max():.4f}, min key {key.min():.4f}")
    assert t2.max() <= -0.01
    assert (lo == 14.9).all()
    assert key.min() >= 14.9


def test_margin_is_not_idle():
    """Point tiles (one pose): the test fires for samples 0.05 m inside the circle abeam of the record, so the margin
    is a margin and not a second bound."""
    rng = np.random.default_rng(42)
    n = 50_000
    hd = rng.uniform(-np.pi, np.pi, n)
    cx, cy = rng.uniform(-150, 150, n), rng.uniform(-150, 150, n)
    side = rng.choice([-1.0, 1.0], n)
    phi = np.deg2rad(rng.uniform(-60, 60, n))  # around the circle centre, from the side away from the record
    r = float(RHO) - 0.05
    lx, ly = r * np.sin(phi), side * (float(RHO) + r * np.cos(phi))  # in the node frame
    sx = cx + lx * np.cos(hd) - ly * np.sin(hd)
    sy = cy + lx * np.sin(hd) + ly * np.cos(hd)
    z = np.zeros(n)
    assert _fire(cx, cy, hd, z, z, sx, sy).mean() > 0.9


def test_near_misses_do_not_fire():
    rng = np.random.default_rng(43)
    n = 200_000
    hd = rng.uniform(-np.pi, np.pi, n)
    cx, cy = rng.uniform(-150, 150, n), rng.uniform(-150, 150, n)
    side = rng.choice([-1.0, 1.0], n)
    # around the circle's centre, from the side away from the record; not within 30 degrees of the record itself,
    # where a point just outside this circle lies inside the other one
    phi = np.deg2rad(rng.uniform(-150, 150, n))

    def at(r, prn, thn):
        lx, ly = r * np.sin(phi), side * (float(RHO) + r * np.cos(phi))
        sx = cx + lx * np.cos(hd) - ly * np.sin(hd)
        sy = cy + lx * np.sin(hd) + ly * np.cos(hd)
        return _fire(cx, cy, hd, prn, thn, sx, sy)

    z = np.zeros(n)
    # the sample on the centre record's circle +- 0.02 m: outside it, on it, and -- a disc of 0.05 m holds a record
    # whose circle excludes the sample -- inside it
    assert not at(float(RHO) + 0.02 * rng.uniform(0, 1, n), z, z).any()
    assert not at(float(RHO) + 0.02 * rng.uniform(-1, 1, n), z + 0.05, z).any()
    assert not at(float(RHO) + 0.02 * rng.uniform(-1, 1, n), z + 0.05, z + np.deg2rad(5)).any()
    # bmax reaching pi (and bmin reaching 0): the sample within A of straight behind / ahead of the mean heading
    for base in (np.pi, 0.0):
        D = rng.uniform(0.3, 12.0, n)
        prn = rng.uniform(0, 0.5, n) * np.minimum(D, 1.0)
        thn = np.deg2rad(rng.uniform(0, 40.0, n))
        A = np.arcsin(np.minimum(prn / D, 1.0)) + thn
        brg = base + side * A * rng.uniform(0, 1, n)
        sx, sy = cx + D * np.cos(hd + brg), cy + D * np.sin(hd + brg)
        assert not _fire(cx, cy, hd, prn, thn, sx, sy).any()
    # D <= pr: the sample inside the disc
    prn = rng.uniform(0.3, 3.0, n)
    D = prn * rng.uniform(0, 1, n)
    brg = rng.uniform(-np.pi, np.pi, n)
    sx, sy = cx + D * np.cos(hd + brg), cy + D * np.sin(hd + brg)
    assert not _fire(cx, cy, hd, prn, z, sx, sy).any()


# ---------------------------------------------------------------------------------------------------------------
# GPU
NS = 256  # samples per class
_GPU = {}


def _clustered(seed=21):
    """~3000 nodes in 64 clusters of 32-64: poses within 0.2 m and 3 degrees inside a cluster (whole tiles with small
    discs and arcs), every fourth cluster of equal poses (runs), every tenth cheap in costE.  Two clusters in three
    look sideways (ang_par 70-90 degrees off the heading, to `side`), so a sample abeam of them passes feasibleNode
    and only the key decides; the others look ahead."""
    import clrrt  # noqa: F401
    from clrrt import abi
    rs = np.random.RandomState(seed)
    clusters, recs = [], []
    for k in range(64):
        x, y, th = rs.uniform(2.0, 60.0), rs.uniform(-10.0, 10.0), rs.uniform(-np.pi, np.pi)
        side = rs.choice([-1.0, 1.0])
        ap_off = side * np.deg2rad(rs.uniform(70.0, 90.0)) if k % 3 else 0.0
        dist = float(np.hypot(x, y))
        ce = 0.5 * dist if k % 10 == 0 else 2.0 + dist * rs.uniform(1.3, 2.0)
        clusters.append((x, y, th, side))
        for _ in range(rs.randint(32, 65)):
            if k % 4 == 1:
                recs.append((x, y, th, th + ap_off, ce))
            else:
                a, r = rs.uniform(-np.pi, np.pi), 0.2 * np.sqrt(rs.uniform())
                dth = np.deg2rad(rs.uniform(-3.0, 3.0))
                recs.append((x + r * np.cos(a), y + r * np.sin(a), th + dth, th + dth + ap_off,
                             ce + rs.uniform(0.0, 0.3)))
    order = rs.permutation(len(recs))  # ids carry no place order
    nodes = (abi.Node * (1 + len(recs)))()
    nodes[0].parent = -1
    nodes[0].ref_front[0], nodes[0].ref_front[1] = -1.0, 0.0
    for i, j in enumerate(order, start=1):
        x, y, th, ap, ce = recs[j]
        d = nodes[i]
        d.parent = 0
        d.state[0], d.state[1], d.state[2] = x, y, th
        d.ref_back[0], d.ref_back[1] = x, y
        d.ref_front[0], d.ref_front[1] = x - np.cos(th), y - np.sin(th)
        d.ref_vback = 1.0
        d.ang_par = float(ap)
        d.costE = np.float32(ce)
    return nodes, clusters


def _cluster_samples(clusters, seed=22):
    """Per class (256 optimize, then 256 explore): 96 abeam of a cluster at 0.3-1.5 rho lateral offset (inside a
    turning circle), 64 on a circle's boundary +- 0.02 m, 64 straight ahead at 1-6 m, 32 behind."""
    from clrrt import abi
    rs = np.random.RandomState(seed)
    rho = float(RHO)
    out = []
    for ex in (0, 1):
        pts = []
        for i in range(NS):
            x, y, th, side = clusters[rs.randint(len(clusters))]
            if i < 96:
                lx, ly = rs.uniform(-1.0, 1.0), side * rho * rs.uniform(0.3, 1.5)
            elif i < 160:
                phi, r = rs.uniform(-np.pi, np.pi), rho + rs.uniform(-0.02, 0.02)
                lx, ly = r * np.sin(phi), side * (rho + r * np.cos(phi))
            elif i < 224:
                lx, ly = rs.uniform(1.0, 6.0), rs.uniform(-0.2, 0.2)
            else:
                lx, ly = -rs.uniform(1.0, 6.0), rs.uniform(-0.5, 0.5)
            pts.append((x + lx * np.cos(th) - ly * np.sin(th), y + lx * np.sin(th) + ly * np.cos(th)))
        out += [abi.Sample(float(px), float(py), ex, 0) for px, py in pts]
    return out


def _gpu_case(sort_limit):
    """(tree, samples, brute-force lists in BATCH and EXACT order), computed once per sort_limit."""
    from test_walk_root_seed import _brute, _lists, _planner
    if "tree" not in _GPU:
        nodes, clusters = _clustered()
        _GPU["tree"] = (nodes, _cluster_samples(clusters))
    if sort_limit not in _GPU:
        nodes, smp = _GPU["tree"]
        pl = _planner(nodes, sort_limit)
        try:
            _brute(pl)
            _GPU[sort_limit] = _lists(pl, smp)
        finally:
            pl.close()
    return _GPU["tree"] + (_GPU[sort_limit],)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True], ids=["walk", "split"])
@pytest.mark.parametrize("sort_limit", [4, 10])
def test_clustered_lists_match_brute_force(sort_limit, split):
    from test_walk_root_seed import _assert_lists_equal, _lists, _planner, _walk
    nodes, smp, ref = _gpu_case(sort_limit)
    ids = ref[0][0]
    n_list = (ids >= 0).sum(axis=1)
    # what the cases are for: abeam explore samples have lists (feasible nodes beside them), all of inside-circle
    # keys there; ahead samples have near keys
    abeam_ex = slice(NS, NS + 96)
    assert (n_list[abeam_ex] > 0).sum() > 48
    assert (ref[0][1][abeam_ex][:, 0][n_list[abeam_ex] > 0] < 14.9).any()
    assert (ref[0][1][NS + 160:NS + 224][:, 0] < 6.5).sum() > 32
    pl = _planner(nodes, sort_limit)
    try:
        _walk(pl, split=split)
        pl.reset_counters()
        got = _lists(pl, smp)
        w = pl.search_work()
        print(f"sort_limit {sort_limit}, split {split}: {w}; overflow records {pl.debug_counters()[32]}")
        if split:
            assert pl.debug_counters()[32] > 0
        _assert_lists_equal(ref, got, f"clustered tree, sort_limit {sort_limit}, split {split}")
    finally:
        pl.close()


_PLAIN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("batch,rounds", [(96, 8), (2048, 5)])
@pytest.mark.parametrize("defer", [0, 128])
def test_trees_equal_unpipelined_rounds(batch, rounds, defer):
    """Lag-2 rounds on the walk (whole-tree index, the appended-node walk, the range index of deferred rounds) grow,
    byte for byte, the tree of unpipelined rounds."""
    from test_nn_delta_walk import _grow
    rows = 1 << 25 if batch > 512 else 1 << 23
    key = (batch, rounds, defer)
    if key not in _PLAIN:
        _PLAIN[key] = _grow(dict(nn_pipeline=0, defer_steps=defer), batch, rounds, max_rows=rows)[:3]
    raw, rws, n, _ = _grow(dict(nn_walk_min=64, nn_lag=2, defer_steps=defer), batch, rounds, max_rows=rows)
    print(f"batch {batch} x {rounds}, defer_steps {defer}: {n} nodes")
    assert n > batch // 2
    assert (raw, rws, n) == _PLAIN[key]
