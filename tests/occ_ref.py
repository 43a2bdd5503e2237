"""numpy restatement of the occupancy-grid decision of CLRRT_COLLISION_OCC (include/clrrt.h, clrrt_set_occupancy).

A grid: corner (x0, y0) of cell (0, 0), cell size res, cells[j, i] != 0 occupied, inflate.  The centre of cell (i, j)
is c = (x0 + (i + 0.5) res, y0 + (j + 0.5) res).  For a state x: vp = (x[0] + 1.424 cos x[2], x[1] + 1.424 sin x[2]),
d = c - vp, u = d.x cos + d.y sin, v = d.y cos - d.x sin; the grid hits when some occupied cell has
|u| <= 2.424 + inflate and |v| <= 1 + inflate.  A non-finite vp or heading does not hit.  All in double, in the
operation order written here (the engine builds without FMA contraction, so only the cosine and sine can differ
from it, by an ulp: the borderline band below).
"""
from collections import namedtuple

import numpy as np

A, B, OFF = 2.424, 1.0, 1.424
BORDER = 1e-9  # |margin| within this: borderline (the only states a GPU test may skip)

Grid = namedtuple("Grid", "x0 y0 res cells inflate")


def default_inflate(res):
    return res * np.sqrt(2.0) / 2.0


def _vp(states):
    st = np.asarray(states, dtype=np.float64).reshape(-1, 10)
    th = st[:, 2]
    with np.errstate(invalid="ignore"):
        c, s = np.cos(th), np.sin(th)
        vpx, vpy = st[:, 0] + OFF * c, st[:, 1] + OFF * s
    ok = np.isfinite(vpx) & np.isfinite(vpy) & np.isfinite(th)
    return vpx, vpy, c, s, ok


def margin(states, grid, tile=8.0):
    """Per state: min over the occupied cells of max(|u| - (A + inflate), |v| - (B + inflate)); +inf where vp or the
    heading is not finite or no occupied cell is near.  hits == (margin <= 0).  The states are binned into square
    tiles and each tile is evaluated against the occupied cells within the box's reach of it only (a cell farther
    than that from a state has a margin above res there: neither a hit nor borderline)."""
    vpx, vpy, c, s, ok = _vp(states)
    a, b = A + grid.inflate, B + grid.inflate
    out = np.full(len(vpx), np.inf)
    jj, ii = np.nonzero(np.asarray(grid.cells))
    if len(ii) == 0 or not ok.any():
        return out
    cx = grid.x0 + (ii + 0.5) * grid.res
    cy = grid.y0 + (jj + 0.5) * grid.res
    reach = np.hypot(a, b) + grid.res
    near = ok & (vpx > cx.min() - reach) & (vpx < cx.max() + reach) & (vpy > cy.min() - reach) & (vpy < cy.max() + reach)
    idx = np.nonzero(near)[0]
    if len(idx) == 0:
        return out
    tx = np.floor(vpx[idx] / tile).astype(np.int64)
    ty = np.floor(vpy[idx] / tile).astype(np.int64)
    order = np.lexsort((ty, tx))
    idx, tx, ty = idx[order], tx[order], ty[order]
    cut = np.nonzero((np.diff(tx) != 0) | (np.diff(ty) != 0))[0] + 1
    for g in np.split(np.arange(len(idx)), cut):
        k = idx[g]
        x0, y0 = tx[g[0]] * tile, ty[g[0]] * tile
        sel = (cx >= x0 - reach) & (cx <= x0 + tile + reach) & (cy >= y0 - reach) & (cy <= y0 + tile + reach)
        if not sel.any():
            continue
        ccx, ccy = cx[sel], cy[sel]
        step = max(1, 2_000_000 // len(ccx))
        for q in range(0, len(k), step):
            kk = k[q:q + step]
            dx = ccx[None, :] - vpx[kk, None]
            dy = ccy[None, :] - vpy[kk, None]
            u = dx * c[kk, None] + dy * s[kk, None]
            v = dy * c[kk, None] - dx * s[kk, None]
            out[kk] = np.maximum(np.abs(u) - a, np.abs(v) - b).min(axis=1)
    return out


def hits(states, grid):
    return margin(states, grid) <= 0.0


def borderline(states, grid):
    return np.abs(margin(states, grid)) <= BORDER


def hits_loop(states, grid):
    """The definition as a plain triple loop (states, rows, columns)."""
    import math
    st = np.asarray(states, dtype=np.float64).reshape(-1, 10)
    cells = np.asarray(grid.cells)
    h, w = cells.shape
    a, b = A + grid.inflate, B + grid.inflate
    out = np.zeros(len(st), dtype=bool)
    for n, x in enumerate(st):
        th = float(x[2])
        if not math.isfinite(th):
            continue
        c, s = float(np.cos(th)), float(np.sin(th))
        vpx, vpy = float(x[0]) + OFF * c, float(x[1]) + OFF * s
        if not (math.isfinite(vpx) and math.isfinite(vpy)):
            continue
        for j in range(h):
            for i in range(w):
                if cells[j, i] == 0:
                    continue
                dx = (grid.x0 + (i + 0.5) * grid.res) - vpx
                dy = (grid.y0 + (j + 0.5) * grid.res) - vpy
                u = dx * c + dy * s
                v = dy * c - dx * s
                if abs(u) <= a and abs(v) <= b:
                    out[n] = True
    return out


def first_hit_row(rows, grid):
    """Index of the first of rows[1:] (a rollout's rows after its start state) that hits, or -1; and whether any row
    before or at it is borderline."""
    if len(rows) < 2:
        return -1, False
    m = margin(rows[1:], grid)
    hit = np.nonzero(m <= 0.0)[0]
    k = int(hit[0]) + 1 if len(hit) else -1
    upto = m if k < 0 else m[:k]
    return k, bool((np.abs(upto) <= BORDER).any())
