"""The restated libm as compiled for the device (clrrt_selftest_math) against the host libm, bit for bit, at every
branch edge the restatement has: the edge sets and sweeps of math_cases.py, in mixed and in uniform waves, at
launch shapes with partial blocks, and against the recorded bits of tests/golden/math_edges.npz (so a GPU host
with another glibc shows as "host differs from golden", not as a device failure).  Arguments outside the restated
domain go to the GPU math library: NaN / inf / sign must agree with libm and their distance is printed, not
bounded."""
import os
import re

import numpy as np
import pytest

import clrrt
import libm_ref
import math_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{fn}-{mc.NAMES[fn]}" for fn in mc.FNS]
SINCOS_LIKE = {fn for fn in mc.FNS if mc.FAMILY[fn] == "sincos"} | {24, 25, 26, 27}


def _block_size():
    src = open(os.path.join(ROOT, "cl-rrt_amd", "csrc", "clrrt_kernels.hip")).read()
    body = src[src.index("hipError_t launch_selftest_math("):]
    m = re.search(r"k_selftest_math, dim3\(\(n \+ (\d+)\) / (\d+)\), dim3\((\d+)\)", body)
    assert m and int(m.group(1)) + 1 == int(m.group(2)) == int(m.group(3))
    return int(m.group(3))


@pytest.fixture(scope="module")
def planner():
    pl = clrrt.Planner(clrrt.default_params(), max_nodes=4, max_rows=4, max_batch=1)
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(mc.GOLDEN_PATH) as z:
        return {k: z[k] for k in z.files}


_DEV = {}


def _device_edges(pl, fn):
    """The device's values on fn's edge set in generator order (computed once per module)."""
    if fn not in _DEV:
        a, b, _ = mc.edge_cases(fn)
        out = pl.selftest_math(fn, a, b)
        out.setflags(write=False)
        _DEV[fn] = out
    return _DEV[fn]


def _assert_same(fn, a, b, got, want, what):
    bad = libm_ref.mismatches(got, want)
    assert len(bad) == 0, f"{what}: " + libm_ref.describe(mc.NAMES[fn], bad, a, b, got, want, "device")


@pytest.mark.parametrize("fn", mc.FNS, ids=IDS)
def test_device_edges(planner, golden, fn):
    a, b, dom = mc.edge_cases(fn)
    g = _device_edges(planner, fn)
    h = libm_ref.eval_libm(fn, a, b)
    _assert_same(fn, a[dom], b[dom], g[dom], h[dom], "device vs host libm, in domain")
    # the recorded bits: first the host against them, then the device
    ga, gb, want = mc.golden_cases(fn, golden)
    idx = mc.golden_index(mc.FAMILY[fn])
    assert np.array_equal(libm_ref.bits(ga), libm_ref.bits(a[idx])) and np.array_equal(libm_ref.bits(gb), libm_ref.bits(b[idx]))
    bad = libm_ref.mismatches(h[idx], want)
    assert len(bad) == 0, "host libm differs from golden (another glibc?): " + libm_ref.describe(
        mc.NAMES[fn], bad, ga, gb, h[idx], want, "host")
    d = dom[idx]
    _assert_same(fn, ga[d], gb[d], g[idx][d], want[d], "device vs golden, in domain")
    # outside the restated domain: the GPU math library's values
    if not dom.all():
        go, ho = g[~dom], h[~dom]
        assert np.array_equal(np.isnan(go), np.isnan(ho)), mc.NAMES[fn]
        assert np.array_equal(np.isinf(go), np.isinf(ho)), mc.NAMES[fn]
        ok = ~np.isnan(ho)
        assert np.array_equal(np.signbit(go[ok]), np.signbit(ho[ok])), mc.NAMES[fn]
        if fn in SINCOS_LIKE:
            assert np.all(np.abs(go[ok]) <= 1.0), mc.NAMES[fn]
        dist = libm_ref.ulp_distance(go, ho)
        print(f"out-of-domain {mc.NAMES[fn]}: {int((~dom).sum())} cases, largest distance to libm "
              f"{int(dist.max())} ulp, differing {int((dist > 0).sum())}")


@pytest.mark.parametrize("fn", mc.FNS, ids=IDS)
def test_device_sweep(planner, fn):
    a, b = mc.sweep(fn)
    assert len(a) == 1 << 20
    _assert_same(fn, a, b, planner.selftest_math(fn, a, b), libm_ref.eval_libm(fn, a, b), "sweep")


@pytest.mark.parametrize("fn", mc.FNS, ids=IDS)
def test_lane_order(planner, fn):
    """Shuffled (every wave mixes the range cases) and sorted by magnitude (uniform waves): the same bits."""
    a, b, _ = mc.edge_cases(fn)
    base = _device_edges(planner, fn)
    perm = np.random.default_rng(1234 + fn).permutation(len(a))
    key = np.abs(b) if fn == 28 else np.abs(a)
    order = np.argsort(np.where(np.isnan(key), np.inf, key), kind="stable")
    for name, p in (("shuffled", perm), ("sorted", order)):
        out = np.empty_like(base)
        out[p] = planner.selftest_math(fn, a[p], b[p])
        assert np.array_equal(libm_ref.bits(out), libm_ref.bits(base)), f"{mc.NAMES[fn]} {name} vs generator order"
    # the shuffle does mix: a wave of 64 holds several of the function's ranges
    if mc.FAMILY[fn] in ("sincos", "step"):
        hi = (a[perm][:64 * 64].view(np.uint64) >> np.uint64(32)).astype(np.int64) & 0x7fffffff
        ranges = np.searchsorted(np.array(mc.SIN_HI_THRESHOLDS), hi, side="right").reshape(64, 64)
        kinds = [len(set(r.tolist())) for r in ranges]
        assert min(kinds) >= 2 and np.mean(kinds) >= 3


@pytest.mark.parametrize("fn", mc.FNS, ids=IDS)
def test_launch_shapes(planner, fn):
    """One lane, one lane short of and past a wave, a partial last block: every block stages the tables before
    its lanes past n leave."""
    block = _block_size()
    a, b, dom = mc.edge_cases(fn)
    base = _device_edges(planner, fn)
    pick = np.random.default_rng(99 + fn).permutation(np.flatnonzero(dom))
    h = libm_ref.eval_libm(fn, a[pick[:4 * block]], b[pick[:4 * block]])
    at = 0
    for n in (1, 1, 1, 1, 63, 65, block - 1, block + 1, 3 * block + 37):
        assert n in (1, 63, 65) or n % block != 0
        idx = pick[at % (4 * block - n):][:n]
        off = at % (4 * block - n)
        out = planner.selftest_math(fn, a[idx], b[idx])
        assert np.array_equal(libm_ref.bits(out), libm_ref.bits(base[idx])), (mc.NAMES[fn], n)
        _assert_same(fn, a[idx], b[idx], out, h[off:off + n], f"n = {n}")
        at += 17
