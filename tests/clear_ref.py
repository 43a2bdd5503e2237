"""numpy restatement of the occupancy clearance (include/clrrt.h, clrrt_set_occupancy_clearance), and the state sets
the clearance tests share (tests/test_clear_host.py checks their input conditions on the CPU, tests/test_clear_gpu.py
runs them on the device).

Field: f[j, i] = min over occupied cells (i', j') of (i - i')^2 + (j - j')^2, uint32, 0xFFFFFFFF with no occupied cell
-- here a brute force over the occupied cells.

Clearance of a state x: cs, sn = cos, sin of x[2]; vp = (x[0] + 1.424 cs, x[1] + 1.424 sn); circle centres
p_k = vp + s_k (cs, sn), s_k in {-1.616, 0.0, +1.616}; f_x = (p_k.x - x0) / res, f_y = (p_k.y - y0) / res; inside when
0 <= f_x < w and 0 <= f_y < h; d_k = res sqrt(f[int(f_y), int(f_x)]) inside, +inf otherwise or with no occupied cell;
c = min_k d_k - (RC + inflate), then min(c, clear_max), then max(c, 0).  All in double, in this order.  The value is a
table lookup, so numpy's cosine and sine -- which may differ from the engine's by an ulp -- move it only where a circle
centre lies on a cell boundary: a state is borderline when a centre's f_x or f_y is within 1e-9 of a cell boundary of
the grid (an integer in [0, w] resp. [0, h]) AND moving the cosine or the sine by one ulp changes a cell that is read
(a car driving along a grid line with heading 0 sits on a boundary exactly, in numpy and in the engine alike: not
borderline).  Only borderline states may be skipped by a GPU comparison.
"""
import numpy as np

from occ_ref import OFF

RC = 1.2857
SK = (-1.616, 0.0, 1.616)
NONE = 0xFFFFFFFF
BORDER = 1e-9
N_EXTRA = 512


def field_at(cells, jy, ix):
    """The field's values at cells (jy[k], ix[k]): a brute force over the occupied cells."""
    jy = np.asarray(jy, dtype=np.int64)
    ix = np.asarray(ix, dtype=np.int64)
    oj, oi = np.nonzero(np.asarray(cells))
    out = np.full(jy.shape, NONE, dtype=np.uint32)
    if len(oi) == 0 or jy.size == 0:
        return out
    best = np.full(jy.shape, np.iinfo(np.int64).max, dtype=np.int64)
    step = max(1, 4_000_000 // jy.size)
    for q in range(0, len(oi), step):
        d = (ix[..., None] - oi[q:q + step]) ** 2 + (jy[..., None] - oj[q:q + step]) ** 2
        best = np.minimum(best, d.min(axis=-1))
    return best.astype(np.uint32)


def field(cells):
    """The whole field, uint32 [h, w]."""
    h, w = np.asarray(cells).shape
    jy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return field_at(cells, jy, ix)


def _centres(states, grid, dc=0, ds=0):
    """Per circle k: (f_x, f_y, inside) of its centre, and the states whose vp and heading are finite.  dc, ds: -1 / +1
    moves the cosine / sine one ulp down / up."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 10)
    h, w = np.asarray(grid.cells).shape
    th = st[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        cs, sn = np.cos(th), np.sin(th)
        if dc:
            cs = np.nextafter(cs, dc * np.inf)
        if ds:
            sn = np.nextafter(sn, ds * np.inf)
        vpx, vpy = st[:, 0] + OFF * cs, st[:, 1] + OFF * sn
        ok = np.isfinite(vpx) & np.isfinite(vpy) & np.isfinite(th)
        out = []
        for s in SK:
            px, py = vpx + s * cs, vpy + s * sn
            fx, fy = (px - grid.x0) / grid.res, (py - grid.y0) / grid.res
            out.append((fx, fy, ok & (fx >= 0.0) & (fx < w) & (fy >= 0.0) & (fy < h)))
    return out, ok


def clearance(states, grid, clear_max):
    cen, _ = _centres(states, grid)
    m = np.full(len(cen[0][0]), np.inf)
    for fx, fy, inside in cen:
        k = np.nonzero(inside)[0]
        f = field_at(grid.cells, fy[k].astype(np.int64), fx[k].astype(np.int64))
        d = np.where(f == NONE, np.inf, grid.res * np.sqrt(f.astype(np.float64)))
        m[k] = np.minimum(m[k], d)
    c = m - (RC + grid.inflate)
    c = np.minimum(c, clear_max)
    return np.maximum(c, 0.0)


def _cells_read(cen):
    """Per circle: the cell index read, -1 outside the grid."""
    out = []
    for fx, fy, inside in cen:
        with np.errstate(invalid="ignore"):
            ix = np.where(inside, fx, 0.0).astype(np.int64)
            jy = np.where(inside, fy, 0.0).astype(np.int64)
        out.append(np.where(inside, jy * (1 << 20) + ix, -1))
    return np.stack(out)


def borderline(states, grid):
    cen, ok = _centres(states, grid)
    h, w = np.asarray(grid.cells).shape
    near = np.zeros(len(ok), dtype=bool)
    with np.errstate(invalid="ignore"):
        for fx, fy, _ in cen:
            for f, n in ((fx, w), (fy, h)):
                r = np.rint(f)
                near |= ok & (np.abs(f - r) <= BORDER) & (r >= 0) & (r <= n)
    if not near.any():
        return near
    base = _cells_read(cen)
    moved = np.zeros(len(ok), dtype=bool)
    for dc in (-1, 0, 1):
        for ds in (-1, 0, 1):
            if dc or ds:
                moved |= (_cells_read(_centres(states, grid, dc, ds)[0]) != base).any(axis=0)
    return near & moved


def _state(vpx, vpy, th):
    st = np.zeros((len(vpx), 10))
    st[:, 0] = vpx - OFF * np.cos(th)
    st[:, 1] = vpy - OFF * np.sin(th)
    st[:, 2] = th
    st[:, 6] = 0.5
    return st


def extra_states(name, grid):
    """512 more states for a grid: a circle centre 1e-6 cell either side of a cell boundary (128 in x, 128 in y), of
    each of the grid's four edges (128), of the switch between which circle is nearest an occupied cell (96: the cell
    on the bisector of two neighbouring centres; grid edges instead when no cell is occupied), and 32 non-finite."""
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    h, w = np.asarray(grid.cells).shape
    oj, oi = np.nonzero(np.asarray(grid.cells))
    n_sw = 96 if len(oi) else 0
    n_cx, n_cy, n_nan = 128, 128, 32
    n_edge = N_EXTRA - n_cx - n_cy - n_nan - n_sw

    def place(fx, fy):  # states with circle k's centre at cell coordinates (fx, fy)
        n = len(fx)
        th = rng.uniform(-np.pi, np.pi, n)
        s = np.asarray(SK)[rng.integers(0, 3, n)]
        px, py = grid.x0 + fx * grid.res, grid.y0 + fy * grid.res
        return _state(px - s * np.cos(th), py - s * np.sin(th), th)

    def side(n):
        return rng.choice([-1e-6, 1e-6], n)

    parts = [place(rng.integers(1, max(w, 2), n_cx) + side(n_cx), rng.uniform(0.0, h, n_cx)),
             place(rng.uniform(0.0, w, n_cy), rng.integers(1, max(h, 2), n_cy) + side(n_cy))]
    q = n_edge // 4
    parts += [place(0.0 + side(q), rng.uniform(0.0, h, q)), place(w + side(q), rng.uniform(0.0, h, q)),
              place(rng.uniform(0.0, w, q), 0.0 + side(q)),
              place(rng.uniform(0.0, w, n_edge - 3 * q), h + side(n_edge - 3 * q))]
    if n_sw:
        pick = rng.integers(0, len(oi), n_sw)
        th = rng.uniform(-np.pi, np.pi, n_sw)
        u = rng.choice([-0.808, 0.808], n_sw) + side(n_sw) * grid.res  # along the axis, from vp to the cell
        v = rng.uniform(-3.0, 3.0, n_sw)
        c, s = np.cos(th), np.sin(th)
        cx, cy = grid.x0 + (oi[pick] + 0.5) * grid.res, grid.y0 + (oj[pick] + 0.5) * grid.res
        parts.append(_state(cx - (u * c - v * s), cy - (u * s + v * c), th))
    bad = place(rng.uniform(0.0, w, n_nan), rng.uniform(0.0, h, n_nan))
    for k, val in enumerate((np.nan, np.inf, -np.inf)):
        bad[k::9, 0] = val
        bad[k + 3::9, 1] = val
        bad[k + 6::9, 2] = val
    parts.append(bad)
    st = np.concatenate(parts)
    assert st.shape == (N_EXTRA, 10), st.shape
    return st
