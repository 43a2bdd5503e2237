"""Writes tests/golden/math_edges.npz: for the edge sets of tests/math_cases.py (thinned as golden_index says;
never the threshold lists), the arguments and the bits the host libm (glibc 2.35) returns for every fn code of
clrrt_selftest_math.  Run from the repository root: python tests/golden/make_math_edges.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libm_ref  # noqa: E402
import math_cases as mc  # noqa: E402


def records():
    out = {}
    for fam in mc.FAMILIES:
        a, b = mc.family_cases(fam)
        idx = mc.golden_index(fam)
        out[f"{fam}.a"] = a[idx].view(np.uint64)
        if np.any(b[idx] != 0.0):
            out[f"{fam}.b"] = b[idx].view(np.uint64)
    for fn in mc.FNS:
        if fn in mc.GOLDEN_FN:
            continue
        a, b = mc.family_cases(mc.FAMILY[fn])
        idx = mc.golden_index(mc.FAMILY[fn])
        out[mc.golden_key(fn)] = mc.golden_pack(fn, libm_ref.eval_libm(fn, a[idx], b[idx]))
    return out


if __name__ == "__main__":
    np.savez_compressed(mc.GOLDEN_PATH, **records())
    print(mc.GOLDEN_PATH, os.path.getsize(mc.GOLDEN_PATH), "bytes")
