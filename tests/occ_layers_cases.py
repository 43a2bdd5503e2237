"""Stacks, times and state sets shared by the layered occupancy tests (tests/test_occ_layers_host.py checks their input
conditions on the CPU, tests/test_occ_layers_gpu.py runs them on the device).  Built on tests/occ_cases.py's grids and
state sets; everything is seeded."""
import numpy as np

import occ_cases
import occ_ref
from occ_ref import Grid

T0, DT = 0.25, 0.5  # k DT and T0 + k DT are exact doubles for k <= 16: time has no borderline band


def times():
    """The time values written round-robin into x[6]: the 17 boundaries T0 + k DT, k = 0 .. 16, their neighbours one
    ulp either side, a time before the stack, one beyond its end, NaN and both infinities (56 values)."""
    b = T0 + np.arange(17) * DT
    return np.concatenate([b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf),
                           [T0 - 1.0, T0 + 20.0 * DT, np.nan, np.inf, -np.inf]])


def _shifted(cells, k, axis, step):
    return np.roll(cells, k * step, axis=axis)


def stacks():
    """name -> (base case of occ_cases.grids(), [Grid per layer]).  The K = 3 stacks shift the base grid's cell, row or
    column from layer to layer; the K = 16 stack draws each layer's fill with its own seed (layer 0: the base's)."""
    g = {n: v[0] for n, v in occ_cases.grids().items()}
    out = {}
    out["k3_one_cell"] = ("one_cell", [g["one_cell"]._replace(cells=_shifted(g["one_cell"].cells, k, 1, 3))
                                       for k in range(3)])
    out["k3_full_row"] = ("full_row", [g["full_row"]._replace(cells=_shifted(g["full_row"].cells, k, 0, 4))
                                       for k in range(3)])
    out["k3_full_col"] = ("full_col", [g["full_col"]._replace(cells=_shifted(g["full_col"].cells, k, 1, -3))
                                       for k in range(3)])
    r = g["random_96x64"]
    out["k16_random"] = ("random_96x64", [r._replace(cells=occ_cases._random_fill(64, 96, 0.05, 7 + 100 * k))
                                          for k in range(16)])
    return out


def cells3d(grids):
    return np.stack([np.asarray(g.cells) for g in grids])


def states(name):
    """The base case's 4096 states with x[6] overwritten round-robin by times()."""
    base, grids = stacks()[name]
    st = occ_cases.states(base, grids[0]).copy()
    tt = times()
    st[:, 6] = tt[np.arange(len(st)) % len(tt)]
    return st


# ---------------------------------------------------------------------------------------------- the gate
GATE_K = 8
GATE_SWITCH = 4  # the gap's state changes at layer 4: t = T0 + 4 DT = 2.25 s
GATE_V0, GATE_VMAX = 7.0, 10.0  # the root's speed: the first rollouts reach the wall plane before the gate switches
WALL_X = 16.0


GAPS = {"gap_1_5": (1.0, 5.0), "gap_m3_3": (-3.0, 3.0)}  # occ_cases.wall_with_gap's own gap, and one astride the x axis


def gate(closing=True, gap="gap_1_5"):
    """wall_with_gap as a stack of GATE_K layers: closing -- the gap is open in layers 0 .. 3 and filled from layer 4
    on; opening -- the reverse.  Few of the rollout jobs steer through the default gap beside the axis; most of those
    that cross the wall plane go through the one astride it."""
    open_g = occ_cases.wall_with_gap(gap=GAPS[gap])
    cells = open_g.cells.copy()
    col = cells.any(axis=0)
    cells[:, col] = 1
    shut_g = open_g._replace(cells=cells)
    first, then = (open_g, shut_g) if closing else (shut_g, open_g)
    return [first if k < GATE_SWITCH else then for k in range(GATE_K)]


def gate_root():
    root = np.zeros(10)
    root[4] = GATE_V0
    return root


def gate_params(mode, **kw):
    import clrrt
    return clrrt.default_params(v0=GATE_V0, vmax=GATE_VMAX, collision_mode=mode, **kw)
