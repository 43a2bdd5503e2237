"""Occupancy clearance (clrrt_set_occupancy_clearance), host side -- CPU only.

* the numpy reference (tests/clear_ref.py) against the definition as plain loops;
* the header declares the four entry points and still defines ABI 11; the binding's record matches the header; the
  library exports the entry points;
* the input conditions of the GPU tests (tests/test_clear_gpu.py), checked with numpy alone.  Each grid of
  occ_cases.grids() has two state sets: the 4096 states of occ_cases.states and the 512 of clear_ref.extra_states
  (circle centres 1e-6 cell either side of a cell boundary, of the grid's four edges and of the switch between which
  circle is nearest, and non-finite states).  At most 1 % of each set is borderline (a circle centre within 1e-9 cell
  of a cell boundary: the only states a GPU comparison may skip), and each set of a grid with an occupied cell has
  clearances at 0, strictly between 0 and clear_max, and at clear_max, for both values of clear_max the GPU test uses.
  (The empty grid is in the GPU cases because every state must read clear_max there; that is asserted instead.)
"""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import clrrt
import clear_ref
import occ_cases
import occ_ref
from clrrt import abi

FUNCS = ("clrrt_set_occupancy_clearance", "clrrt_occupancy_clearance_info", "clrrt_occupancy_field",
         "clrrt_occupancy_clearance")


def test_field_matches_plain_loops():
    rng = np.random.default_rng(2)
    cells = (rng.random((7, 9)) < 0.15).astype(np.uint8)
    cells[3, 4] = 1
    f = clear_ref.field(cells)
    assert f.dtype == np.uint32 and f.shape == cells.shape
    occ = [(i, j) for j in range(7) for i in range(9) if cells[j, i]]
    for j in range(7):
        for i in range(9):
            assert f[j, i] == min((i - a) ** 2 + (j - b) ** 2 for a, b in occ), (i, j)
    assert (clear_ref.field(np.zeros((3, 5), np.uint8)) == 0xFFFFFFFF).all()


def test_clearance_matches_plain_loops():
    rng = np.random.default_rng(3)
    cells = (rng.random((12, 16)) < 0.05).astype(np.uint8)
    cells[5, 9] = 1
    for inflate, clear_max in ((0.0, 3.0), (0.3, 0.5)):
        g = occ_ref.Grid(1.0, -3.0, 0.5, cells, inflate)
        f = clear_ref.field(cells)
        st = np.zeros((400, 10))
        st[:, 0] = rng.uniform(-6.0, 14.0, 400)
        st[:, 1] = rng.uniform(-9.0, 9.0, 400)
        st[:, 2] = rng.uniform(-4.0, 4.0, 400)
        st[::50, 0] = np.nan
        st[7::50, 2] = np.inf
        st[11::50, 1] = -1e300
        got = clear_ref.clearance(st, g, clear_max)
        for n, x in enumerate(st):
            d = math.inf
            th = float(x[2])
            if math.isfinite(th):
                cs, sn = float(np.cos(th)), float(np.sin(th))
                vpx, vpy = float(x[0]) + 1.424 * cs, float(x[1]) + 1.424 * sn
                if math.isfinite(vpx) and math.isfinite(vpy):
                    for s in (-1.616, 0.0, 1.616):
                        fx, fy = (vpx + s * cs - g.x0) / g.res, (vpy + s * sn - g.y0) / g.res
                        if 0 <= fx < 16 and 0 <= fy < 12:
                            d = min(d, g.res * math.sqrt(float(f[int(fy), int(fx)])))
            c = max(min(d - (1.2857 + inflate), clear_max), 0.0)
            assert got[n] == c, (n, got[n], c)
        assert (got[::50] == clear_max).all() and (got[7::50] == clear_max).all() and (got[11::50] == clear_max).all()
        assert (got == 0).any() and ((got > 0) & (got < clear_max)).any() and (got == clear_max).any()
    g0 = occ_ref.Grid(1.0, -3.0, 0.5, np.zeros((12, 16), np.uint8), 0.0)
    assert (clear_ref.clearance(st, g0, 2.0) == 2.0).all()


def test_the_circles_cover_the_vehicle_box():
    # a point of the 4.848 x 2 box is at most 0.808 along and 1 across from the nearest circle centre
    assert math.hypot(1.616 / 2, 1.0) <= clear_ref.RC and 3 * 1.616 == pytest.approx(2 * occ_ref.A)


def test_header_declares_the_entry_points_and_keeps_abi_11():
    txt = open(clrrt.HEADER_PATH).read()
    assert re.search(r"#define\s+CLRRT_ABI_VERSION\s+11\b", txt) and abi.CLRRT_ABI_VERSION == 11
    for name in FUNCS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in clrrt.exported_symbols()
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "clrrt.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(clrrt_clearance_info_t), offsetof(clrrt_clearance_info_t, clear_max),
         offsetof(clrrt_clearance_info_t, on), offsetof(clrrt_clearance_info_t, baked),
         offsetof(clrrt_clearance_info_t, field_bytes), offsetof(clrrt_clearance_info_t, bake_ms));
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
    ci = abi.ClearanceInfo
    assert got[:6] == [C.sizeof(ci), ci.clear_max.offset, ci.on.offset, ci.baked.offset, ci.field_bytes.offset,
                       ci.bake_ms.offset]
    assert got[6:] == [40, 48] == [C.sizeof(abi.Occupancy), C.sizeof(abi.OccupancyInfo)]


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", clrrt.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in FUNCS:
        assert name in exported, name
    assert clrrt.lib().clrrt_abi_version() == 11


def test_bad_arguments_are_refused_before_any_device_call():
    L = clrrt.lib()
    assert L.clrrt_set_occupancy_clearance(None, 1.0) == -1
    assert L.clrrt_occupancy_clearance_info(None, None) == -1
    assert L.clrrt_occupancy_field(None, None) == -1
    assert L.clrrt_occupancy_clearance(None, None, 0, None) == -1


def test_adapter_and_native_program_compile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "clrrt_adapter.hpp")).read()
    assert len(re.findall(r"void\s+setOccupancyClearance\s*\(\s*double", txt)) == 2  # MotionPlanner and the wrapper
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "native", "occ_clearance.cpp")], check=True)


_sets = {}


def sets(name):
    """(grid, {set name: states}) of a grid of occ_cases.grids()."""
    if name not in _sets:
        g, _ = occ_cases.grids()[name]
        _sets[name] = (g, {"states": occ_cases.states(name, g), "extra": clear_ref.extra_states(name, g)})
    return _sets[name]


@pytest.mark.parametrize("name", list(occ_cases.grids()))
def test_gpu_state_sets_meet_their_input_conditions(name):
    g, ss = sets(name)
    assert ss["states"].shape == (4096, 10) and ss["extra"].shape == (512, 10)
    for label, st in ss.items():
        border = clear_ref.borderline(st, g)
        assert border.mean() <= 0.01, (label, border.sum())
        assert not np.isfinite(st).all()  # the non-finite states are in
        for clear_max in (3.0, 0.5):
            c = clear_ref.clearance(st, g, clear_max)
            n0, nm, n1 = (c == 0).sum(), ((c > 0) & (c < clear_max)).sum(), (c == clear_max).sum()
            print(f"{name}/{label} clear_max {clear_max}: {n0} at 0, {nm} between, {n1} at clear_max, "
                  f"{border.sum()} borderline")
            assert n0 + nm + n1 == len(st)
            if np.count_nonzero(g.cells) == 0:
                assert n1 == len(st)
            else:
                assert n0 > 0 and nm > 0 and n1 > 0, (label, clear_max)
    # the extra states sit where they are meant to: the first 384 (cell boundaries and grid edges) have a centre
    # within 2e-6 cell of a boundary, and are not borderline for it
    cen, ok = clear_ref._centres(ss["extra"], g)
    near = np.zeros(len(ok), bool)
    with np.errstate(invalid="ignore"):
        for fx, fy, _ in cen:
            near |= ok & ((np.abs(fx - np.rint(fx)) < 2e-6) | (np.abs(fy - np.rint(fy)) < 2e-6))
    assert near[:384].all() and not clear_ref.borderline(ss["extra"], g)[:384].any()
