"""The host build of the restated libm (clrrt_glibc.hpp, clrrt_glibcf.hpp) against the host libm, bit for bit, for
every fn code of clrrt_selftest_math on the edge sets of math_cases.py and on 2^20-argument sweeps -- the
case-selected and branch-free forms the rollout step evaluates (sincos_sel, sin_cos_fma_sel, step_trig) included.
CPU only; test_math_edges_gpu.py asks the same of the compiled device code."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import libm_ref
import math_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cl-rrt_amd", "csrc")


def _ids(fns):
    return [f"{fn}-{mc.NAMES[fn]}" for fn in fns]


def test_constants_are_the_headers():
    data = open(os.path.join(CSRC, "clrrt_glibc_data.hpp")).read()
    for name in ("big", "hp0", "taylor_lim", "tan_g1", "tan_g2", "tan_g3", "two8", "mfftnhf", "at_inv16"):
        m = re.search(rf"constexpr double {name} = (\S+);", data)
        assert m and float.fromhex(m.group(1)) == getattr(mc, name), name
    for name in ("SINCOSTAB_N", "XFG_ROWS", "ATAN2_CIJ_ROWS"):
        m = re.search(rf"constexpr int {name} = (\d+);", data)
        assert m and int(m.group(1)) == getattr(mc, name), name
    code = open(os.path.join(CSRC, "clrrt_glibc.hpp")).read()
    for t in mc.SIN_HI_THRESHOLDS:
        assert f"{t:#010x}u" in code, hex(t)
    assert f"|x| < {int(mc.SIN_DOMAIN_END)} for sin/cos" in code
    for t in mc.EXP_TOP12:
        assert f"{t:#x}" in code, hex(t)
    codef = open(os.path.join(CSRC, "clrrt_glibcf.hpp")).read().lower()
    for t in set(mc.ACOSF_WORDS + mc.ASINF_WORDS + mc.ATANF_WORDS):
        assert f"{t:#010x}" in codef, hex(t)
    sp = re.search(r"const double sp\[\] = \{(.*?)\};", open(os.path.join(ROOT, "tests", "native", "atan2_check.cpp")).read(),
                   re.S).group(1)
    names = {"INFINITY": np.inf, "-INFINITY": -np.inf, "NAN": np.nan}
    vals = [names[t] if t in names else float(t) for t in (t.strip() for t in sp.split(","))]
    assert np.array_equal(libm_ref.bits(vals), libm_ref.bits(mc.ATAN2_SP))


def test_exp_thresholds_are_libms():
    """The copied overflow / subnormal / zero bounds of exp are where the host libm changes behaviour."""
    e = lambda x: float(libm_ref.eval_libm(6, [x])[0])  # noqa: E731
    up, dn = np.nextafter(mc.EXP_OVERFLOW, np.inf), np.nextafter(mc.EXP_ZERO, -np.inf)
    assert np.isfinite(e(mc.EXP_OVERFLOW)) and np.isinf(e(up))
    assert e(mc.EXP_ZERO) == 5e-324 and e(dn) == 0.0
    assert e(mc.EXP_SUBNORMAL) >= 2.2250738585072014e-308 > e(np.nextafter(mc.EXP_SUBNORMAL, -np.inf))


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_edge_sets_are_deterministic_and_in_domain(family):
    a, b = mc.family_cases(family)
    assert len(a) == len(b) == sum(n for _, n in mc.segments(family))
    for fn in (f for f in mc.FNS if mc.FAMILY[f] == family):
        _, _, dom = mc.edge_cases(fn)  # asserts the share itself
        assert dom.mean() >= 0.99
        h = libm_ref.eval_libm(fn, a, b)
        # the reference on the in-domain cases: finite, or the same special value whoever computes it
        assert not np.any(np.isnan(h[dom]) & ~np.isnan(libm_ref.eval_restated(fn, a, b)[dom]))
    a2, b2 = mc._BUILDERS[family]().arrays()
    assert np.array_equal(libm_ref.bits(a), libm_ref.bits(a2)) and np.array_equal(libm_ref.bits(b), libm_ref.bits(b2))


def test_edge_sets_reach_every_branch():
    """The sets put cases on both sides of every threshold they name (a guard against a generator edit that
    silently loses a list)."""
    a, _ = mc.family_cases("sincos")
    hi = (a.view(np.uint64) >> np.uint64(32)).astype(np.int64) & 0x7fffffff
    for t in mc.SIN_HI_THRESHOLDS:
        assert {t - 1, t, t + 1} <= set(hi.tolist()), hex(t)
    k = (np.abs(a[np.abs(a) < 0.855]) + mc.big).view(np.uint64) & np.uint64(0xffffffff)
    assert set(k.tolist()) >= set(range(mc.SINCOSTAB_N // 4))  # every sincostab row as a direct argument
    t, _ = mc.family_cases("tan")
    w = np.abs(t[(np.abs(t) > mc.tan_g2) & (np.abs(t) <= mc.tan_g3)])
    assert set((w * mc.two8 + mc.mfftnhf).astype(int).tolist()) == set(range(mc.XFG_ROWS))  # every xfg row
    for g in (mc.tan_g1, mc.tan_g2, mc.tan_g3):
        assert np.any(t == g) and np.any(t == np.nextafter(g, 0)) and np.any(t == np.nextafter(g, 1))
    y, x = mc.family_cases("atan2")
    with np.errstate(all="ignore"):
        u = np.minimum(np.abs(y), np.abs(x)) / np.maximum(np.abs(y), np.abs(x))
    u = u[np.isfinite(u) & (u >= mc.at_inv16) & (u <= 1)]
    assert set(((u * 256 + 2.0 ** 52) - 2.0 ** 52 - 16).astype(int).tolist()) == set(range(mc.ATAN2_CIJ_ROWS))
    e, _ = mc.family_cases("exp")
    assert np.any(e == mc.EXP_OVERFLOW) and np.any(e == mc.EXP_ZERO) and np.any(np.isinf(e)) and np.any(np.isnan(e))
    f, _ = mc.family_cases("float1")
    f32 = f.astype(np.float32)
    assert np.sum((f32 != 0) & (np.abs(f32) < np.float32(1.1754944e-38))) > 1000  # subnormal float inputs


@pytest.mark.parametrize("fn", mc.FNS, ids=_ids(mc.FNS))
def test_restated_vs_libm_edges(fn):
    a, b, dom = mc.edge_cases(fn)
    a, b = a[dom], b[dom]
    r, h = libm_ref.eval_restated(fn, a, b), libm_ref.eval_libm(fn, a, b)
    bad = libm_ref.mismatches(r, h)
    assert len(bad) == 0, libm_ref.describe(mc.NAMES[fn], bad, a, b, r, h, "restated")


@pytest.mark.parametrize("fn", mc.FNS, ids=_ids(mc.FNS))
def test_restated_vs_libm_sweep(fn):
    a, b = mc.sweep(fn)
    assert len(a) == 1 << 20
    r, h = libm_ref.eval_restated(fn, a, b), libm_ref.eval_libm(fn, a, b)
    bad = libm_ref.mismatches(r, h)
    assert len(bad) == 0, libm_ref.describe(mc.NAMES[fn], bad, a, b, r, h, "restated")


def test_step_trig_fallback_gives_the_block_its_bits():
    """step_trig.* with one argument outside the block's domain (the hook then evaluates sincos_sel,
    sin_cos_fma_sel and tan) equals the same function with both arguments inside it."""
    a, b = mc.family_cases("step")
    sin_in, tan_in = mc.in_domain(24, a, b), mc.in_domain(28, a, b)
    x3_out, x2_out = sin_in & ~tan_in, ~sin_in & tan_in
    assert x3_out.sum() >= 100 and x2_out.sum() >= 20
    for fn in (24, 25, 26, 27):
        inside = libm_ref.eval_restated(fn, a[x3_out], np.zeros(int(x3_out.sum())))
        assert len(libm_ref.mismatches(libm_ref.eval_restated(fn, a[x3_out], b[x3_out]), inside)) == 0, mc.NAMES[fn]
    inside = libm_ref.eval_restated(28, np.zeros(int(x2_out.sum())), b[x2_out])
    assert len(libm_ref.mismatches(libm_ref.eval_restated(28, a[x2_out], b[x2_out]), inside)) == 0


def test_golden_math_edges_is_current():
    """tests/golden/math_edges.npz holds what the generators and this libm give, wherever tools/gen_glibc_libm.py
    accepts the libm image (the gate of test_glibc_data_header_is_current)."""
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_glibc_libm.py"), "--out", os.path.join(td, "h.hpp")],
                       check=True, capture_output=True)
    assert os.path.getsize(mc.GOLDEN_PATH) < (1 << 20)
    with np.load(mc.GOLDEN_PATH) as z:
        for fam in mc.FAMILIES:
            a, b = mc.family_cases(fam)
            idx = mc.golden_index(fam)
            # thinning never touches a threshold list: segments kept whole are there in full
            assert np.array_equal(z[f"{fam}.a"], a[idx].view(np.uint64)), fam
            if f"{fam}.b" in z:
                assert np.array_equal(z[f"{fam}.b"], b[idx].view(np.uint64)), fam
            else:
                assert not np.any(b[idx] != 0.0), fam
        for fn in mc.FNS:
            a, b, want = mc.golden_cases(fn, z)
            h = libm_ref.eval_libm(fn, a, b)
            bad = libm_ref.mismatches(h, want)
            assert len(bad) == 0, "host libm differs from golden: " + libm_ref.describe(mc.NAMES[fn], bad, a, b, h, want, "host")
