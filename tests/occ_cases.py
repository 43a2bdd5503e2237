"""Grids and state sets shared by the occupancy-grid tests (tests/test_occ_host.py checks their input conditions on the
CPU, tests/test_occ_gpu.py runs them on the device).  Everything is seeded: both files see the same arrays."""
import numpy as np

import occ_ref
from occ_ref import A, B, OFF, Grid

N_STATES = 4096


def _random_fill(h, w, share, seed):
    return (np.random.default_rng(seed).random((h, w)) < share).astype(np.uint8)


def grids():
    """name -> (Grid, expected placement 'lds' / 'global').  The inflate values cover 0, the binding's default
    (res sqrt 2 / 2) and a value above the cell size."""
    out = {}
    out["empty"] = (Grid(5.0, -6.0, 0.5, np.zeros((24, 40), np.uint8), 0.0), "lds")
    one = np.zeros((24, 40), np.uint8)
    one[11, 17] = 1
    out["one_cell"] = (Grid(5.0, -6.0, 0.5, one, occ_ref.default_inflate(0.5)), "lds")
    row = np.zeros((30, 40), np.uint8)
    row[10, :] = 1
    out["full_row"] = (Grid(4.0, -7.0, 0.5, row, 0.0), "lds")
    col = np.zeros((30, 41), np.uint8)  # 41: a row that is no multiple of the 32-bit words
    col[:, 33] = 1
    out["full_col"] = (Grid(4.0, -7.0, 0.5, col, 0.3), "lds")
    out["random_96x64"] = (Grid(10.0, -8.0, 0.25, _random_fill(64, 96, 0.05, 7), occ_ref.default_inflate(0.25)), "lds")
    out["random_1024"] = (Grid(-20.0, -51.2, 0.1, _random_fill(1024, 1024, 0.01, 8), 0.0), "global")
    return out


def _state(vpx, vpy, th):
    st = np.zeros((len(vpx), 10))
    st[:, 0] = vpx - OFF * np.cos(th)
    st[:, 1] = vpy - OFF * np.sin(th)
    st[:, 2] = th
    st[:, 6] = 0.5
    return st


def states(name, grid):
    """4096 states for a grid: uniform over a region around the occupied cells (the whole grid when none is), states
    just outside each grid edge, far-away and non-finite ones, and near-contact states 1e-6 m either side of each of
    the four box faces and of a corner of an occupied cell."""
    rng = np.random.default_rng(sum(map(ord, name)))
    h, w = grid.cells.shape
    jj, ii = np.nonzero(grid.cells)
    gx0, gx1 = grid.x0, grid.x0 + w * grid.res
    gy0, gy1 = grid.y0, grid.y0 + h * grid.res
    if len(ii):
        cx = grid.x0 + (ii + 0.5) * grid.res
        cy = grid.y0 + (jj + 0.5) * grid.res
        # a region whose share of hitting states is well inside [0.1, 0.9]: a sparse set of cells gets a close frame,
        # a filled grid (where nearly every inside state hits) a frame wider than the grid
        dense = len(ii) > 4 * max(h, w)
        pad = 0.35 * max(gx1 - gx0, gy1 - gy0) if dense else 3.5
        rx0, rx1, ry0, ry1 = cx.min() - pad, cx.max() + pad, cy.min() - pad, cy.max() + pad
    else:
        rx0, rx1, ry0, ry1 = gx0 - 4.0, gx1 + 4.0, gy0 - 4.0, gy1 + 4.0
    parts = []
    n_edge, n_far, n_nan, n_near = 256, 128, 64, 450 if len(ii) else 0
    n_uni = N_STATES - n_edge - n_far - n_nan - n_near
    parts.append(_state(rng.uniform(rx0, rx1, n_uni), rng.uniform(ry0, ry1, n_uni), rng.uniform(-np.pi, np.pi, n_uni)))
    # just outside each grid edge (vp up to 3 m out)
    q = n_edge // 4
    out = rng.uniform(0.0, 3.0, q)
    parts.append(_state(gx0 - out, rng.uniform(gy0, gy1, q), rng.uniform(-np.pi, np.pi, q)))
    parts.append(_state(gx1 + out, rng.uniform(gy0, gy1, q), rng.uniform(-np.pi, np.pi, q)))
    parts.append(_state(rng.uniform(gx0, gx1, q), gy0 - out, rng.uniform(-np.pi, np.pi, q)))
    parts.append(_state(rng.uniform(gx0, gx1, q), gy1 + out, rng.uniform(-np.pi, np.pi, q)))
    # far away
    mag = 10.0 ** rng.uniform(3.0, 12.0, n_far) * rng.choice([-1.0, 1.0], n_far)
    far = _state(mag, mag[::-1].copy(), rng.uniform(-np.pi, np.pi, n_far))
    far[:8, 0] = 1e300
    far[8:16, 1] = -1e300
    parts.append(far)
    # non-finite position or heading
    bad = _state(rng.uniform(rx0, rx1, n_nan), rng.uniform(ry0, ry1, n_nan), rng.uniform(-np.pi, np.pi, n_nan))
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        bad[k::9, 0] = v
        bad[k + 3::9, 1] = v
        bad[k + 6::9, 2] = v
    parts.append(bad)
    if n_near:
        a, b = A + grid.inflate, B + grid.inflate
        pick = rng.integers(0, len(ii), n_near)
        th = rng.uniform(-np.pi, np.pi, n_near)
        dlt = rng.choice([-1e-6, 1e-6], n_near)
        sgn = rng.choice([-1.0, 1.0], n_near)
        kind = np.arange(n_near) % 5  # 0, 1: the two u faces; 2, 3: the two v faces; 4: a corner
        u = np.where(kind < 2, np.where(kind == 0, 1.0, -1.0) * (a + dlt), rng.uniform(-0.9 * a, 0.9 * a, n_near))
        v = np.where((kind == 2) | (kind == 3), np.where(kind == 2, 1.0, -1.0) * (b + dlt),
                     rng.uniform(-0.9 * b, 0.9 * b, n_near))
        corner = kind == 4
        dlt2 = rng.choice([-1e-6, 1e-6], n_near)
        u = np.where(corner, sgn * (a + dlt), u)
        v = np.where(corner, rng.choice([-1.0, 1.0], n_near) * (b + dlt2), v)
        c, s = np.cos(th), np.sin(th)
        # d = c_cell - vp = u (cos, sin) + v (-sin, cos)
        vpx = cx[pick] - (u * c - v * s)
        vpy = cy[pick] - (u * s + v * c)
        parts.append(_state(vpx, vpy, th))
    st = np.concatenate(parts)
    assert st.shape == (N_STATES, 10), st.shape
    return st


def wall_with_gap(x0=0.0, y0=-12.0, res=0.25, w=160, h=96, wall_x=16.0, gap=(1.0, 5.0)):
    """A wall two cells thick across the corridor at x = wall_x with an opening gap[0] <= y < gap[1]."""
    cells = np.zeros((h, w), np.uint8)
    i = int(round((wall_x - x0) / res))
    cy = y0 + (np.arange(h) + 0.5) * res
    cells[(cy < gap[0]) | (cy >= gap[1]), i:i + 2] = 1
    return Grid(x0, y0, res, cells, occ_ref.default_inflate(res))


def rollout_jobs(n=512, seed=3):
    """simulate_batch jobs from the root: samples ahead of the car, on both sides of the wall of wall_with_gap."""
    rng = np.random.default_rng(seed)
    return [(0, 0, float(x), float(y)) for x, y in zip(rng.uniform(6.0, 40.0, n), rng.uniform(-9.0, 9.0, n))]
