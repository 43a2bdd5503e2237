"""Occupancy-grid collision mode (CLRRT_COLLISION_OCC), host side -- CPU only.

* the numpy reference (tests/occ_ref.py) against the definition as a plain triple loop;
* the binding's records against the header, the new entry points exported by the library;
* the input conditions of the GPU tests (tests/test_occ_gpu.py), checked with numpy alone: each state set's share of
  hitting states lies in [0.10, 0.90] and at most 0.1 % of a set is borderline (smallest
  max(|u| - 2.424 - inflate, |v| - 1 - inflate) over the occupied cells within 1e-9 of 0) -- the only states a GPU
  test may skip.  (The empty grid is in the GPU cases because no state may hit it; its share is 0 by construction
  and is asserted to be exactly that.)
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import clrrt
import occ_cases
import occ_ref
from clrrt import abi, scenes


def test_reference_matches_triple_loop():
    rng = np.random.default_rng(1)
    cells = (rng.random((6, 8)) < 0.2).astype(np.uint8)
    cells[2, 5] = 1
    for inflate in (0.0, 0.2):
        g = occ_ref.Grid(1.0, -1.5, 0.5, cells, inflate)
        st = np.zeros((600, 10))
        st[:, 0] = rng.uniform(-6.0, 10.0, 600)
        st[:, 1] = rng.uniform(-7.0, 7.0, 600)
        st[:, 2] = rng.uniform(-4.0, 4.0, 600)
        st[::50, 0] = np.nan
        st[7::50, 2] = np.inf
        st[11::50, 1] = 1e300
        want = occ_ref.hits_loop(st, g)
        got = occ_ref.hits(st, g)
        assert np.array_equal(got, want)
        assert 0.1 < want.mean() < 0.9
        assert not want[::50].any() and not want[7::50].any() and not want[11::50].any()
    # no occupied cell, and a state whose box reaches no cell
    g0 = occ_ref.Grid(1.0, -1.5, 0.5, np.zeros((6, 8), np.uint8), 0.0)
    assert not occ_ref.hits(st, g0).any() and not occ_ref.hits_loop(st[:40], g0).any()


def test_first_hit_row():
    g = occ_cases.wall_with_gap()
    rows = np.zeros((40, 10))
    rows[:, 0] = np.arange(40) * 0.5  # straight along x at y = -3: into the wall
    rows[:, 1] = -3.0
    k, border = occ_ref.first_hit_row(rows, g)
    want = np.nonzero(occ_ref.hits_loop(rows[1:], g))[0][0] + 1
    assert k == want and not border
    rows[:, 1] = 3.0  # through the gap
    assert occ_ref.first_hit_row(rows, g) == (-1, False)


def test_binding_records_match_header():
    txt = open(clrrt.HEADER_PATH).read()
    assert re.search(r"#define\s+CLRRT_COLLISION_OCC\s+2\b", txt) and abi.CLRRT_COLLISION_OCC == 2
    assert re.search(r"#define\s+CLRRT_ABI_VERSION\s+11\b", txt)
    # the header's records, compiled: sizes and field offsets
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "clrrt.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(clrrt_occupancy), offsetof(clrrt_occupancy, res),
         offsetof(clrrt_occupancy, inflate), offsetof(clrrt_occupancy, w), offsetof(clrrt_occupancy, h));
  printf("%zu %zu %zu %zu %zu\n", sizeof(clrrt_occupancy_info_t), offsetof(clrrt_occupancy_info_t, placement),
         offsetof(clrrt_occupancy_info_t, occupied), offsetof(clrrt_occupancy_info_t, map_bytes),
         offsetof(clrrt_occupancy_info_t, bake_ms));
  printf("%d %d %d\n", CLRRT_OCC_NONE, CLRRT_OCC_LDS, CLRRT_OCC_GLOBAL);
  return 0;
}
'''
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(clrrt.HEADER_PATH), "-o", os.path.join(d, "t"),
                        os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in out]
    o, i = abi.Occupancy, abi.OccupancyInfo
    assert got[:5] == [C.sizeof(o), o.res.offset, o.inflate.offset, o.w.offset, o.h.offset]
    assert got[5:10] == [C.sizeof(i), i.placement.offset, i.occupied.offset, i.map_bytes.offset, i.bake_ms.offset]
    assert got[10:] == [abi.OCC_NONE, abi.OCC_LDS, abi.OCC_GLOBAL]


def test_library_exports_occupancy_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", clrrt.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    txt = open(clrrt.HEADER_PATH).read()
    for name in ("clrrt_set_occupancy", "clrrt_occupancy_info"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in exported and name in clrrt.exported_symbols()
    assert clrrt.lib().clrrt_abi_version() == 11


def test_rasterize_marks_centres_inside_static_boxes():
    obs = np.array([[10.0, 2.0, 0.3, 4.0, 8.0, 0.0, 0.0],    # static: half extents 2 along the heading, 1 across
                    [20.0, -3.0, 1.0, 4.0, 8.0, 0.5, 0.0]])  # moving: stays a box
    x0, y0, res, w, h = 0.0, -10.0, 0.25, 120, 80
    cells = scenes.rasterize(obs, x0, y0, res, w, h)
    assert cells.shape == (h, w) and cells.dtype == np.uint8
    c, s = np.cos(0.3), np.sin(0.3)
    n = 0
    for j in range(h):
        for i in range(w):
            dx, dy = x0 + (i + 0.5) * res - 10.0, y0 + (j + 0.5) * res - 2.0
            inside = abs(dx * c + dy * s) <= 2.0 and abs(dy * c - dx * s) <= 1.0
            assert bool(cells[j, i]) == inside, (i, j)
            n += inside
    assert abs(n * res * res - 8.0) < 0.5  # the box's 4 x 2 m


_sets = {}


def _set(name):
    if name not in _sets:
        g, _ = occ_cases.grids()[name]
        st = occ_cases.states(name, g)
        _sets[name] = (g, st, occ_ref.margin(st, g))
    return _sets[name]


@pytest.mark.parametrize("name", list(occ_cases.grids()))
def test_gpu_state_sets_meet_their_input_conditions(name):
    g, st, m = _set(name)
    assert st.shape == (occ_cases.N_STATES, 10)
    share = (m <= 0.0).mean()
    border = (np.abs(m) <= occ_ref.BORDER).mean()
    print(f"{name}: {int(np.count_nonzero(g.cells))} occupied cells, hit share {share:.3f}, borderline {border:.5f}")
    if np.count_nonzero(g.cells) == 0:
        assert share == 0.0
    else:
        assert 0.10 <= share <= 0.90
        # the near-contact states sit 1e-6 m from a face: both sides of the decision occur among them
        # (on the random fills another occupied cell decides nearly all of them: the sparse grids carry this case)
        if name in ("one_cell", "full_row", "full_col"):
            near = m[np.abs(m) < 2e-6]
            assert (near <= 0).sum() >= 20 and (near > 0).sum() >= 20
    assert border <= 0.001
    assert not np.isfinite(st).all()  # the non-finite states are in


def test_rollout_grid_is_a_wall_with_a_gap():
    g = occ_cases.wall_with_gap()
    col = g.cells.any(axis=0)
    assert col.sum() == 2
    wall = g.cells[:, col][:, 0]
    cy = g.y0 + (np.arange(len(wall)) + 0.5) * g.res
    assert not wall[(cy >= 1.0) & (cy < 5.0)].any() and wall[(cy < 1.0) | (cy >= 5.0)].all()
    assert len(occ_cases.rollout_jobs()) == 512
