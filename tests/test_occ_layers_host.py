"""Time-layered occupancy stacks (clrrt_set_occupancy_layers), host side -- CPU only.

* the header declares the new calls and the ABI version is unchanged; the binding declares them and its record matches
  the header's, compiled;
* the layer rule's numpy restatement (tests/occ_layers_ref.py) at the boundaries and one ulp either side;
* the input conditions of the GPU sets (tests/occ_layers_cases.py): per stack every layer is selected by at least 64
  states, the states of each layer hit that layer's grid with a share in [0.1, 0.9], and at most 0.5 % of a set is
  borderline (occ_ref.BORDER) -- the only states a GPU test may skip; time has no borderline band;
* scenes.rasterize_layers against a per-cell loop;
* the gate scene: from the oracle's rows of whole simulations (its rollouts know no grid), which of the 512 rollout jobs
  cross the wall plane while the gap is open and which only afterwards.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import clrrt
import occ_cases
import occ_layers_cases as lc
import occ_layers_ref as lr
import occ_ref
from clrrt import abi, scenes

NEW_CALLS = ("clrrt_set_occupancy_layers", "clrrt_occupancy_layers_info", "clrrt_occupancy_field_layer")


def test_header_declares_the_layer_calls_and_keeps_the_abi_version():
    txt = open(clrrt.HEADER_PATH).read()
    assert re.search(r"#define\s+CLRRT_ABI_VERSION\s+11\b", txt)
    assert re.search(r"#define\s+CLRRT_OCC_REACH_LDS\s+3\b", txt) and abi.OCC_REACH_LDS == 3
    assert re.search(r"#define\s+CLRRT_OCC_MAX_LAYERS\s+16\b", txt) and abi.OCC_MAX_LAYERS == 16
    for name in NEW_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    assert re.search(r"int\s+clrrt_set_occupancy_layers\(clrrt_ctx\*\s*\w*,\s*const clrrt_occupancy\*\s*\w*,\s*int32_t\s+"
                     r"layers,\s*double\s+t0,\s*double\s+dt,\s*const uint8_t\*\s*cells\)", txt)


def test_binding_declares_the_layer_calls_and_its_record_matches():
    out = subprocess.run(["nm", "-D", "--defined-only", clrrt.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in NEW_CALLS:
        assert name in exported and name in clrrt.exported_symbols(), name
        assert getattr(clrrt.lib(), name).argtypes is not None, name
    assert clrrt.lib().clrrt_abi_version() == 11
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "clrrt.h"
int main(void) {
  typedef clrrt_occupancy_layers_info_t T;
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(T), offsetof(T, layers), offsetof(T, placement),
         offsetof(T, t0), offsetof(T, dt), offsetof(T, occupied), offsetof(T, map_bytes),
         offsetof(T, union_reach_bytes), offsetof(T, field_bytes), offsetof(T, bake_ms));
  printf("%zu %zu\n", sizeof(clrrt_occupancy), sizeof(clrrt_occupancy_info_t));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(clrrt.HEADER_PATH), "-o", os.path.join(d, "t"),
                        os.path.join(d, "t.c")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    i = abi.OccupancyLayersInfo
    assert got[:10] == [C.sizeof(i), i.layers.offset, i.placement.offset, i.t0.offset, i.dt.offset, i.occupied.offset,
                        i.map_bytes.offset, i.union_reach_bytes.offset, i.field_bytes.offset, i.bake_ms.offset]
    assert got[10:] == [C.sizeof(abi.Occupancy), C.sizeof(abi.OccupancyInfo)]  # the old records did not change


def test_layer_rule_at_the_boundaries():
    t0, dt = lc.T0, lc.DT
    for K in (1, 3, 8, 16):
        b = t0 + np.arange(17) * dt
        assert np.array_equal((b - t0) / dt, np.arange(17.0))  # exact doubles: no borderline band in time
        at = lr.layer_of(b, t0, dt, K)
        below = lr.layer_of(np.nextafter(b, -np.inf), t0, dt, K)
        above = lr.layer_of(np.nextafter(b, np.inf), t0, dt, K)
        k = np.arange(17)
        assert np.array_equal(at, np.minimum(k, K - 1))
        assert np.array_equal(above, np.minimum(k, K - 1))
        assert np.array_equal(below, np.minimum(np.maximum(k - 1, 0), K - 1))
        odd = lr.layer_of([t0 - 1.0, t0 + 20 * dt, np.nan, np.inf, -np.inf, -1e308, 1e308], t0, dt, K)
        assert odd.tolist() == [0, K - 1, 0, K - 1, 0, 0, K - 1]
        assert not lr.layer_of(lc.times(), t0, dt, K, use_pred=False).any()
    # the plain-Python statement of the rule, value by value
    for K in (3, 16):
        for t in lc.times():
            q = (float(t) - t0) / dt
            want = 0 if not q >= 0 else (K - 1 if q >= K - 1 else int(q))
            assert int(lr.layer_of(t, t0, dt, K)) == want, (t, K)


@pytest.mark.parametrize("name", list(lc.stacks()))
def test_gpu_state_sets_meet_their_input_conditions(name):
    base, grids = lc.stacks()[name]
    K = len(grids)
    st = lc.states(name)
    assert st.shape == (occ_cases.N_STATES, 10) and len(lc.times()) == 56
    for a, b in zip(grids, grids[1:]):
        assert not np.array_equal(a.cells, b.cells)  # the layers differ
        assert (a.x0, a.y0, a.res, a.inflate, a.cells.shape) == (b.x0, b.y0, b.res, b.inflate, b.cells.shape)
    m, k = lr.margin_layers(st, grids, lc.T0, lc.DT)
    border = (np.abs(m) <= occ_ref.BORDER).mean()
    for q in range(K):
        sel = k == q
        share = (m[sel] <= 0.0).mean()
        print(f"{name} layer {q}: {int(sel.sum())} states, hit share {share:.3f}")
        assert sel.sum() >= 64
        assert 0.1 <= share <= 0.9
    print(f"{name}: borderline {border:.5f}")
    assert border <= 0.005
    # the layer decides: testing every state against layer 0 would give another answer for many of them
    m0 = occ_ref.margin(st, grids[0])
    assert ((m0 <= 0) != (m <= 0)).sum() >= 64
    # the states at a boundary, and one ulp either side, select the layers the rule says
    tt = lc.times()
    which = np.arange(len(st)) % len(tt)
    for j in range(17):
        assert (k[which == j] == min(j, K - 1)).all()
        assert (k[which == 17 + j] == min(max(j - 1, 0), K - 1)).all()
        assert (k[which == 34 + j] == min(j, K - 1)).all()
    assert (k[which == 51] == 0).all() and (k[which == 52] == K - 1).all() and (k[which == 53] == 0).all()
    assert (k[which == 54] == K - 1).all() and (k[which == 55] == 0).all()


def test_rasterize_layers_against_a_per_cell_loop():
    obs = np.array([[6.0, 1.0, 0.3, 4.0, 8.0, 0.0, 0.0],     # static
                    [3.0, -1.0, 1.0, 4.0, 6.0, 1.5, -0.5]])  # moving: half extents 1.5 along the heading, 1 across
    x0, y0, res, w, h, K, t0, dt, sub = 0.0, -3.0, 0.5, 20, 12, 3, 0.25, 0.5, 4
    got = scenes.rasterize_layers(obs, x0, y0, res, w, h, K, t0, dt, sub)
    assert got.shape == (K, h, w) and got.dtype == np.uint8
    static = scenes.rasterize(obs, x0, y0, res, w, h)
    c, s = np.cos(1.0), np.sin(1.0)
    for k in range(K):
        for j in range(h):
            for i in range(w):
                inside = bool(static[j, i])
                for q in range(sub + 1):
                    t = t0 + (k + q / sub) * dt
                    dx = x0 + (i + 0.5) * res - (3.0 + 1.5 * t)
                    dy = y0 + (j + 0.5) * res - (-1.0 - 0.5 * t)
                    inside |= abs(dx * c + dy * s) <= 1.5 and abs(dy * c - dx * s) <= 1.0
                assert bool(got[k, j, i]) == inside, (k, i, j)
    assert all((got[k] != got[k + 1]).any() for k in range(K - 1))  # the mover moves
    assert all((got[k] & ~static).sum() >= 8 for k in range(K))
    assert "not a conservative sweep" in scenes.rasterize_layers.__doc__.lower()
    one = scenes.rasterize_layers(obs[:1], x0, y0, res, w, h, 2, t0, dt)  # no mover: every layer is the static grid
    assert np.array_equal(one[0], static) and np.array_equal(one[1], static)


def test_gate_scene_has_rollouts_that_cross_before_and_after_the_switch():
    """The oracle's rows of whole simulations (stub collision: no grid), from the gate's root and parameters."""
    from oracle_binding import Oracle
    o = Oracle(abi.default_params(v0=lc.GATE_V0, vmax=lc.GATE_VMAX))
    o.init_tree(lc.gate_root())
    t_switch = lc.T0 + lc.GATE_SWITCH * lc.DT
    early = late = never = 0
    hits = {(c, g): [0, 0] for c in (True, False) for g in lc.GAPS}
    swayed = {g: 0 for g in lc.GAPS}
    for _, _, x, y in occ_cases.rollout_jobs():
        rows = o.simulate(0, 0, x, y, rows=True, rows_cap=2048)["rows"]
        cross = np.nonzero(rows[:, 0] >= lc.WALL_X)[0]
        if len(cross) == 0:
            never += 1
        elif rows[cross[0], 6] < t_switch:
            early += 1
        else:
            late += 1
        for g in lc.GAPS:
            ks = []
            for closing in (True, False):
                k, _ = lr.first_hit_row(rows, lc.gate(closing, g), lc.T0, lc.DT)
                hits[(closing, g)][k >= 0] += 1
                ks.append(k >= 0)
            swayed[g] += ks[0] != ks[1]
    print(f"cross the wall plane before the switch {early}, only afterwards {late}, never {never}; free/hit per "
          f"(closing, gap) {hits}; rollouts the closing and the opening gate decide differently {swayed}")
    assert early >= 16 and late >= 16
    assert all(min(v) >= 16 for v in hits.values())
    # the rollouts start at one speed, so they reach the wall within a second of each other: the ones the two gates
    # decide differently are those inside the gap when it switches
    assert swayed["gap_m3_3"] >= 8 and swayed["gap_1_5"] >= 1
    # the gate is what it says: open layers have the gap, filled ones a whole wall
    for closing in (True, False):
        g = lc.gate(closing)
        assert len(g) == lc.GATE_K == 8
        full = [bool(q.cells[:, q.cells.any(axis=0)].all()) for q in g]
        assert full == [not closing] * 4 + [closing] * 4
