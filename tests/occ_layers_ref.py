"""numpy restatement of the layer rule of clrrt_set_occupancy_layers (include/clrrt.h): which of a stack's grids a
state is tested against.  The decision against that grid is tests/occ_ref.py's, unchanged.

    t = x[6] under obs_use_pred, else 0;  q = (t - t0) / dt  (float64, a division);
    layer 0 when !(q >= 0) (NaN, -inf),  layer K - 1 when q >= K - 1 (+inf),  else int(q).
"""
import numpy as np

import occ_ref


def layer_of(t, t0, dt, K, use_pred=True):
    t = np.asarray(t, dtype=np.float64)
    if not use_pred:
        t = np.zeros_like(t)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (t - np.float64(t0)) / np.float64(dt)
    k = np.zeros(q.shape, dtype=np.int64)
    top = q >= K - 1
    mid = (q >= 0) & ~top
    k[top] = K - 1
    k[mid] = q[mid].astype(np.int64)
    return k


def margin_layers(states, grids, t0, dt, use_pred=True):
    """occ_ref.margin of each state against the grid of its layer; grids: one occ_ref.Grid per layer.  Returns
    (margin, layer)."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 10)
    k = layer_of(st[:, 6], t0, dt, len(grids), use_pred)
    m = np.full(len(st), np.inf)
    for q, g in enumerate(grids):
        sel = k == q
        if sel.any():
            m[sel] = occ_ref.margin(st[sel], g)
    return m, k


def first_hit_row(rows, grids, t0, dt, use_pred=True):
    """occ_ref.first_hit_row with each row tested against the layer of its own row[6]."""
    if len(rows) < 2:
        return -1, False
    m, _ = margin_layers(rows[1:], grids, t0, dt, use_pred)
    hit = np.nonzero(m <= 0.0)[0]
    k = int(hit[0]) + 1 if len(hit) else -1
    upto = m if k < 0 else m[:k]
    return k, bool((np.abs(upto) <= occ_ref.BORDER).any())
