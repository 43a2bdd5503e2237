"""The walk search's index and key bounds, checked on the compiled device code (clrrt_nnwalk.hip).

The walk prunes with bounds; its lists are exact only while every bound is a lower bound on the float Dubins key of
every record it covers, and the index encloses its records.  Here the index the builders make is downloaded
(clrrt_debug_walk_index) and the bound functions run on the device (clrrt_selftest_walk), against the float key the
searches compute (clrrt_selftest_units: CLRRT_UNIT_DUBINS, CLRRT_UNIT_FEASIBLE, pinned bit for bit to the reference's
code by tests/test_ref_units.py).  The tree and samples are tests/walk_cases.py.

CPU tests: the checkers flag planted violations in a synthetic index made in numpy, and pass the unplanted one.
All checker arithmetic is float64; a tolerance appears only where stated.
"""
import re

import numpy as np
import pytest

import walk_cases as wc

F = np.float32
ROOT_BIT = 0x40000000
ROOT_K, ROOT_SCAN = 64, 16384
ESTATE, ECAPACITY = -4, -3
TILE_FIELDS = ("pcx", "pcy", "pr", "rcx", "rcy", "rr", "thx", "thy", "thh", "apx", "apy", "aph", "cemin", "aopt",
               "nonfinite", "eroot")


# ------------------------------------------------------------------------------------------------------ checkers
def _members(ix, rec):
    """Per place: validity, the exact double fields of its node relative to the frame origin, finiteness of the float
    record (what the builders test)."""
    ids = ix["ID"]
    valid = ids >= 0
    safe = np.where(valid, ids, 0)
    m = {"valid": valid, "id": ids}
    for k, o in (("x", ix["ox"]), ("y", ix["oy"]), ("bx", ix["ox"]), ("by", ix["oy"]), ("h", 0.0), ("ap", 0.0)):
        m[k] = np.where(valid, rec[k][safe] - o, np.nan)
    m["ce"] = np.where(valid, rec["ce"][safe].astype(np.float64), np.nan)
    m["fin"] = valid & np.isfinite(ix["P"]).all(axis=1) & np.isfinite(ix["Q"]).all(axis=1) & np.isfinite(ix["CE"])
    return m


def _same_f32(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32)) or \
        np.array_equal(a, b, equal_nan=True)


def check_records(ix, rec):
    """ID is a permutation of the range, padding is the padding record, P / Q / CE are the float conversions of the
    tree's fields relative to (ox, oy) (the rotations c, s / ca, sa within 3e-7 of the float64 cos / sin: they are
    float libm results of float angles)."""
    bad = []
    n, first = ix["count"], ix["first"]
    ids = ix["ID"]
    if not np.array_equal(np.sort(ids[:n]), np.arange(first, first + n)):
        bad.append("ID[0:count] is not a permutation of the range")
    if not (ids[n:] == -1).all():
        bad.append("padding ids are not -1")
    pad = np.array([0, 0, 1, 0], F)
    if not ((ix["P"][n:] == pad).all() and (ix["Q"][n:] == pad).all() and (ix["CE"][n:] == 0).all()):
        bad.append("padding records differ from (0, 0, 1, 0), costE 0")
    i = ids[:n]
    if np.array_equal(np.sort(i), np.arange(first, first + n)):
        want = {("P", 0): (rec["x"][i] - ix["ox"]).astype(F), ("P", 1): (rec["y"][i] - ix["oy"]).astype(F),
                ("Q", 0): (rec["bx"][i] - ix["ox"]).astype(F), ("Q", 1): (rec["by"][i] - ix["oy"]).astype(F)}
        for (a, c), w in want.items():
            if not _same_f32(ix[a][:n, c], w):
                bad.append(f"{a}[:, {c}] is not the float conversion of the node field")
        if not _same_f32(ix["CE"][:n], rec["ce"][i]):
            bad.append("CE differs from costE")
        h = F(-rec["h"][i]).astype(np.float64)
        ap = F(rec["ap"][i]).astype(np.float64)
        for a, c, w in (("P", 2, np.cos(h)), ("P", 3, np.sin(h)), ("Q", 2, np.cos(ap)), ("Q", 3, np.sin(ap))):
            ok = np.isfinite(w)
            if not (np.abs(ix[a][:n, c][ok] - w[ok]) <= 3e-7).all():
                bad.append(f"{a}[:, {c}] is not the rotation of the node's angle")
    return bad


def expected_heads(ix, rec):
    """Run heads from the records: a record continues its predecessor's run when (x, y, c, s, costE) are equal (exact
    x, y; the rotation as the index holds it); the fused builder cuts runs at super-tile boundaries.  Padding records
    are their own heads.  Returns (head, in root class)."""
    m = _members(ix, rec)
    npad = ix["npad"]
    safe = np.where(m["valid"], m["id"], 0)
    raw = lambda k: np.where(m["valid"], rec[k][safe], np.nan)  # noqa: E731
    key = np.stack([raw("x"), raw("y"), ix["P"][:, 2].astype(np.float64), ix["P"][:, 3].astype(np.float64), m["ce"]], axis=1)
    same = np.zeros(npad, bool)
    same[1:] = (key[1:] == key[:-1]).all(axis=1) & m["valid"][1:] & m["valid"][:-1]
    if ix["fused"]:
        same[::1024] = False
    start = np.where(~same, np.arange(npad), 0)
    head = np.maximum.accumulate(start)
    root = np.zeros(npad, bool)
    if not ix["fused"] and ix["first"] == 0:
        at0 = np.nonzero(ix["ID"] == 0)[0]
        if at0.size:
            root = (key == key[at0[0]]).all(axis=1) & m["valid"]
    return head, root


def check_runs(ix, rec):
    bad = []
    head, root = expected_heads(ix, rec)
    H = ix["HEAD"]
    wrong = np.nonzero((H & ~ROOT_BIT) != head)[0]
    if wrong.size:
        bad.append(f"HEAD: {wrong.size} wrong run heads, first at place {wrong[0]}: {H[wrong[0]] & ~ROOT_BIT} for {head[wrong[0]]}")
    wrong = np.nonzero(((H & ROOT_BIT) != 0) != root)[0]
    if wrong.size:
        bad.append(f"HEAD: root bit wrong at {wrong.size} places, first {wrong[0]}")
    full = head | np.where(root, ROOT_BIT, 0)
    nt = ix["ntiles"]
    h0, h1 = full[::32], full[31::32]
    mid = ix["ID"].reshape(nt, 32).min(axis=1)
    one = (h0 == h1) & (mid >= 0)
    want = np.where(one[:, None], np.stack([h0, mid], axis=1), -1)
    wrong = np.nonzero((ix["trun"] != want).any(axis=1))[0]
    if wrong.size:
        bad.append(f"trun: {wrong.size} tiles wrong, first {wrong[0]}: {ix['trun'][wrong[0]]} for {want[wrong[0]]}")
    return bad


def expected_roster(ix, rec):
    """(count, X, ids): the first min(64, members) ids of node 0's class among [0, min(N, root_scan)), ascending; X =
    the 64th member's id, or the last scanned id with fewer (clrrt_nnwalk.hip header).  Range and fused indexes: none."""
    if ix["fused"] or ix["first"] != 0:
        return 0, -1, np.zeros(0, np.int64)
    nscan = min(ix["count"], ROOT_SCAN)
    # node 0's class by the exact fields (equal headings give equal rotations)
    cls = np.nonzero((rec["x"][:nscan] == rec["x"][0]) & (rec["y"][:nscan] == rec["y"][0]) &
                     (rec["h"][:nscan] == rec["h"][0]) & (rec["ce"][:nscan] == rec["ce"][0]))[0]
    if cls.size >= ROOT_K:
        return ROOT_K, int(cls[ROOT_K - 1]), cls[:ROOT_K]
    return cls.size, nscan - 1, cls


def check_roster(ix, rec):
    n, X, ids = expected_roster(ix, rec)
    r = ix["roster"]
    bad = []
    if r[0] != n or r[1] != X:
        bad.append(f"roster: (entries, X) = ({r[0]}, {r[1]}) for ({n}, {X})")
    elif not np.array_equal(r[2:2 + n], ids):
        k = int(np.nonzero(r[2:2 + n] != ids)[0][0])
        bad.append(f"roster: entry {k} is {r[2 + k]}, the class's {k}-th id is {ids[k]}")
    return bad


def frame_extent(ix):
    """E of nn_setup from its delta = 16 * 2^-24 E + 1e-5: every frame coordinate is below E in size."""
    return (ix["delta"] - 1e-5) * 2.0 ** 20


def check_bounds(ix, rec, which, stats=None):
    """The per-tile (which = 'tiles', 32 records) or per-super-tile ('supers', 1024) bounds against the exact double
    positions minus (ox, oy).  No tolerance: the code carries its own margins.

    Not vacuous: pr (rr) is at most the exact enclosing radius about its centre with the builder's own inflation --
    relative 1e-5, 2 slack, 1e-5 -- plus float rounding 2^-22 E: the member's float coordinates each err by <= 2^-25 E
    (half an ulp below E), <= 2^-24 E in the distance, and the differences, squares, sum, square root and the
    inflation are <= 6 roundings of values below E / 2, 3 * 2^-24 E.  thh (aph) is at most 2e-3 plus acos's value at
    cos(t) - e, t the exact half-arc about its centre and e = 8 * 2^-24 the error of the float dot product (unit vectors
    and the rotation each within an ulp of 1, the normalising division, the centre's length; acos answers it with
    e / sin t, up to sqrt(2 e) = 1e-3 at both ends of its range), plus 1e-6 in the angle: the float angle of the record
    (half an ulp below 4, 1.2e-7), acosf's result (an ulp, 2.4e-7) and the float sum with 2e-3 (1.2e-7)."""
    W = ix[which]
    size = 32 if which == "tiles" else 1024
    n = len(W)
    m = _members(ix, rec)
    sh = (n, size)
    fin = m["fin"].reshape(sh)
    anyf = fin.any(axis=1)
    f = {k: W[k].astype(np.float64) for k in TILE_FIELDS}
    slack, E = ix["slack"], frame_extent(ix)
    bad = []

    def worst(v, over):  # max over the finite members
        return np.where(fin, v, -np.inf).max(axis=1) if over == "max" else np.where(fin, v, np.inf).min(axis=1)

    def report(name, cond, detail=""):
        t = np.nonzero(cond)[0]
        if t.size:
            bad.append(f"{which}: {name} at {t.size} of {n}, first {t[0]} {detail}")

    px, py, bx, by = (m[k].reshape(sh) for k in ("x", "y", "bx", "by"))
    ce = m["ce"].reshape(sh)
    dp = np.hypot(px - f["pcx"][:, None], py - f["pcy"][:, None])
    dr = np.hypot(bx - f["rcx"][:, None], by - f["rcy"][:, None])
    rp, rr = worst(dp, "max"), worst(dr, "max")
    report("a member outside the position disc", anyf & (rp > f["pr"]))
    report("a ref.back() outside its disc", anyf & (rr > f["rr"]))
    report("pr = rr = -1 not exactly where no member is finite", ((f["pr"] == -1) != ~anyf) | ((f["rr"] == -1) != ~anyf) |
           (anyf & ((f["pr"] < 0) | (f["rr"] < 0))))
    arcs = {}
    for ang, cx, cy, hw, name in (("h", "thx", "thy", "thh", "heading"), ("ap", "apx", "apy", "aph", "ang_par")):
        a = m[ang].reshape(sh)
        nrm = np.hypot(f[cx], f[cy])
        dot = (np.cos(a) * f[cx][:, None] + np.sin(a) * f[cy][:, None]) / nrm[:, None]
        t = worst(np.arccos(np.clip(dot, -1.0, 1.0)), "max")
        arcs[hw] = t
        report(f"a {name} outside its arc", anyf & (f[hw] < 3) & (t > f[hw]))
    report("cemin above the smallest costE", anyf & (f["cemin"] > worst(ce, "min")))
    report("aopt above min(costE - |p - c|)", anyf & (f["aopt"] > worst(ce - dp, "min")))
    dR = np.hypot(px - ix["R"][0], py - ix["R"][1])
    report("eroot above min(costE - |p - R|)", anyf & (f["eroot"] > worst(ce - dR, "min")))
    nonf = (m["valid"] & ~m["fin"]).reshape(sh).any(axis=1)
    report("nonfinite flag wrong", (W["nonfinite"] != 0) != nonf)
    # not vacuous
    rnd = 2.0 ** -22 * E
    ex_p = np.where(anyf, f["pr"] - (rp * (1 + 1e-5) + 2 * slack + 1e-5 + rnd), -np.inf)
    ex_r = np.where(anyf, f["rr"] - (rr * (1 + 1e-5) + 2 * slack + 1e-5 + rnd), -np.inf)
    report("pr wider than the enclosing radius and the builder's inflation", ex_p > 0, f"excess {ex_p.max():.3g}")
    report("rr wider than the enclosing radius and the builder's inflation", ex_r > 0, f"excess {ex_r.max():.3g}")
    e = 8 * 2.0 ** -24
    ex_a = []
    for hw in ("thh", "aph"):
        t = arcs[hw]
        with np.errstate(invalid="ignore"):  # (tiles without a finite member: t = -inf, masked below)
            lim = np.arccos(np.maximum(np.cos(t) - e, -1.0)) + 2e-3 + 1e-6
        x = np.where(anyf & (f[hw] < 3.99), f[hw] - lim, -np.inf)
        ex_a.append(x.max())
        report(f"{hw} wider than the exact half-arc and the builder's margin", x > 0,
               f"excess {x.max():.3g} at half-arc {t[int(np.argmax(x))]:.6f}, {hw} {f[hw][int(np.argmax(x))]:.6f}")
    if stats is not None:
        stats[which] = {"pr": ex_p.max(), "rr": ex_r.max(), "thh": ex_a[0], "aph": ex_a[1],
                        "unbounded_th": int((anyf & (f["thh"] >= 3)).sum()), "unbounded_ap": int((anyf & (f["aph"] >= 3)).sum()),
                        "nonfinite": int(nonf.sum()), "empty": int((~anyf).sum())}
    return bad


def check_index(ix, rec, stats=None):
    return (check_records(ix, rec) + check_runs(ix, rec) + check_roster(ix, rec) +
            check_bounds(ix, rec, "tiles", stats) + check_bounds(ix, rec, "supers", stats))


# ------------------------------------------------------------------------------------------- synthetic index (CPU)
def _up(v):
    return np.nextafter(np.asarray(v, np.float64).astype(F), F(np.inf))


def _down(v):
    return np.nextafter(np.asarray(v, np.float64).astype(F), F(-np.inf))


TILE_DTYPE = np.dtype([(k, np.int32 if k == "nonfinite" else F) for k in TILE_FIELDS])


def synth_index(rec, first, count, fused, ox=25.0, oy=0.0, slack=6.5e-5):
    """A valid index of nodes [first, first + count) made in numpy: records in the order of their key inputs, run
    heads by a plain loop, every bound from the exact values with the builder's margins, rounded outwards."""
    ids = first + np.lexsort((rec["ce"][first:first + count], rec["h"][first:first + count],
                              rec["y"][first:first + count], rec["x"][first:first + count]))
    npad = (count + 1023) // 1024 * 1024
    nt, ns = npad // 32, npad // 1024
    P = np.tile(np.array([0, 0, 1, 0], F), (npad, 1))
    Q = P.copy()
    CE = np.zeros(npad, F)
    ID = np.full(npad, -1, np.int32)
    ID[:count] = ids
    h, ap = F(-rec["h"][ids]).astype(np.float64), F(rec["ap"][ids]).astype(np.float64)
    P[:count] = np.stack([rec["x"][ids] - ox, rec["y"][ids] - oy, np.cos(h), np.sin(h)], axis=1).astype(F)
    Q[:count] = np.stack([rec["bx"][ids] - ox, rec["by"][ids] - oy, np.cos(ap), np.sin(ap)], axis=1).astype(F)
    CE[:count] = rec["ce"][ids]
    R = np.array([F(rec["x"][0] - ox), F(rec["y"][0] - oy)], np.float64)
    ix = {"P": P, "Q": Q, "CE": CE, "ID": ID, "npad": npad, "ntiles": nt, "nsup": ns, "ox": ox, "oy": oy,
          "delta": slack, "slack": slack, "R": R, "first": first, "count": count, "fused": bool(fused)}
    rooted = not fused and first == 0
    HEAD = np.arange(npad, dtype=np.int32)
    key = lambda j: (rec["x"][ID[j]], rec["y"][ID[j]], P[j, 2], P[j, 3], CE[j])  # noqa: E731
    k0 = (rec["x"][0], rec["y"][0], float(F(np.cos(F(-rec["h"][0])))), float(F(np.sin(F(-rec["h"][0])))), rec["ce"][0])
    for j in range(count):
        if j > 0 and key(j) == key(j - 1) and not (fused and j % 1024 == 0):
            HEAD[j] = HEAD[j - 1]
        elif rooted and key(j) == k0:
            HEAD[j] = j | ROOT_BIT
    ix["HEAD"] = HEAD
    trun = np.full((nt, 2), -1, np.int32)
    for t in range(nt):
        if HEAD[32 * t] == HEAD[32 * t + 31] and ID[32 * t:32 * t + 32].min() >= 0:
            trun[t] = (HEAD[32 * t], ID[32 * t:32 * t + 32].min())
    ix["trun"] = trun
    n, X, members = expected_roster(ix, rec)  # the rule itself; the plant below removes an id
    roster = np.zeros(66, np.int32)
    roster[0], roster[1] = n, X
    roster[2:2 + n] = members
    ix["roster"] = roster
    m = _members(ix, rec)
    for which, size, cnt in (("tiles", 32, nt), ("supers", 1024, ns)):
        W = np.zeros(cnt, TILE_DTYPE)
        for t in range(cnt):
            sl = slice(t * size, (t + 1) * size)
            fin = m["fin"][sl]
            w = W[t]
            w["nonfinite"] = int((m["valid"][sl] & ~fin).any())
            if not fin.any():
                w["pr"] = w["rr"] = -1
                w["thx"] = w["apx"] = 1
                w["thh"] = w["aph"] = 4
                continue
            x, y, bx, by, hh, aa, ce = (m[k][sl][fin] for k in ("x", "y", "bx", "by", "h", "ap", "ce"))
            w["pcx"], w["pcy"], w["rcx"], w["rcy"] = x.mean(), y.mean(), bx.mean(), by.mean()
            dp = np.hypot(x - float(w["pcx"]), y - float(w["pcy"]))
            dr = np.hypot(bx - float(w["rcx"]), by - float(w["rcy"]))
            w["pr"] = _up(dp.max() * (1 + 1e-5) + 2 * slack + 1e-5)
            w["rr"] = _up(dr.max() * (1 + 1e-5) + 2 * slack + 1e-5)
            for ang, cx, cy, hw in ((hh, "thx", "thy", "thh"), (aa, "apx", "apy", "aph")):
                ux, uy = np.cos(ang).sum(), np.sin(ang).sum()
                if np.hypot(ux, uy) > 1e-3 * ang.size:
                    w[cx], w[cy] = ux / np.hypot(ux, uy), uy / np.hypot(ux, uy)
                    d = (np.cos(ang) * float(w[cx]) + np.sin(ang) * float(w[cy])) / np.hypot(float(w[cx]), float(w[cy]))
                    w[hw] = _up(np.arccos(np.clip(d, -1, 1)).max() + 2e-3)
                else:
                    w[cx], w[cy], w[hw] = 1, 0, 4
            w["cemin"] = ce.min()
            a = (ce - dp).min()
            w["aopt"] = _down(a - 2 * slack - 1e-4 - 1e-5 * abs(a))
            a = (ce - np.hypot(x - R[0], y - R[1])).min()
            w["eroot"] = _down(a - 2 * slack - 1e-4 - 1e-5 * abs(a))
        ix[which] = W
    return ix


def _copy(ix):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ix.items()}


@pytest.fixture(scope="module")
def main_rec():
    return wc.main_tree()


@pytest.fixture(scope="module")
def synth(main_rec):
    rec, _ = main_rec
    return {f: synth_index(rec, 0, wc.N_MAIN, f) for f in (0, 1)}


@pytest.mark.parametrize("fused", [0, 1])
def test_checkers_pass_the_unplanted_index(main_rec, synth, fused):
    stats = {}
    assert check_index(synth[fused], main_rec[0], stats) == []
    assert stats["tiles"]["nonfinite"] >= 1 and stats["tiles"]["empty"] >= 1


def test_checkers_pass_a_synthetic_range_index(main_rec):
    rec, _ = main_rec
    assert check_index(synth_index(rec, 777, 1500, 0), rec) == []


def _finite_tile(ix, need=lambda w: True):
    for t, w in enumerate(ix["tiles"]):
        if w["pr"] >= 0 and need(w):
            return t
    raise AssertionError("no such tile")


@pytest.mark.parametrize("fused", [0, 1])
def test_checkers_flag_planted_violations(main_rec, synth, fused):
    rec, _ = main_rec
    base = synth[fused]

    def flagged(ix, word):
        got = check_index(ix, rec)
        assert got and all(word in g for g in got), got

    ix = _copy(base)
    ix["tiles"]["pr"][_finite_tile(ix)] -= F(1e-3)  # a disc shrunk by 1e-3
    flagged(ix, "tiles: ")
    assert any("position disc" in g or "pr = rr" in g for g in check_index(ix, rec))
    ix = _copy(base)
    ix["supers"]["rr"][0] -= F(1e-3)
    assert any("supers: a ref.back() outside" in g for g in check_index(ix, rec))
    for hw, name in (("thh", "heading"), ("aph", "ang_par")):  # an arc narrowed by 5e-3
        ix = _copy(base)
        ix["tiles"][hw][_finite_tile(ix, lambda w: w[hw] < 3)] -= F(5e-3)
        assert check_index(ix, rec) == [g for g in check_index(ix, rec) if f"a {name} outside its arc" in g] != []
    ix = _copy(base)  # aopt raised by 1e-3 (where its own relative margin is small)
    t = int(np.argmin(np.where(ix["tiles"]["pr"] >= 0, np.abs(ix["tiles"]["aopt"]), np.inf)))
    ix["tiles"]["aopt"][t] += F(1e-3)
    flagged(ix, "aopt above")
    ix = _copy(base)  # eroot likewise
    t = int(np.argmin(np.where(ix["tiles"]["pr"] >= 0, np.abs(ix["tiles"]["eroot"]), np.inf)))
    ix["tiles"]["eroot"][t] += F(1e-3)
    flagged(ix, "eroot above")
    ix = _copy(base)  # a wrong run head: the second record of a run made its own head
    j = int(np.nonzero((ix["HEAD"] & ~ROOT_BIT) != np.arange(ix["npad"]))[0][5])
    ix["HEAD"][j] = j | (ix["HEAD"][j] & ROOT_BIT)
    flagged(ix, "HEAD: ")
    ix = _copy(base)  # a run head without its root bit
    if not fused:
        j = int(np.nonzero(ix["HEAD"] & ROOT_BIT)[0][0])
        ix["HEAD"][j] &= ~ROOT_BIT
        flagged(ix, "root bit")
        ix = _copy(base)  # a roster id missing
        r = ix["roster"]
        later = expected_roster(base, rec)
        cls = np.nonzero((rec["x"] == rec["x"][0]) & (rec["y"] == rec["y"][0]) & (rec["h"] == rec["h"][0]) &
                         (rec["ce"] == rec["ce"][0]))[0]
        assert later[0] == ROOT_K and cls.size > ROOT_K
        r[2 + 5:2 + 63] = r[2 + 6:2 + 64].copy()
        r[2 + 63] = r[1] = cls[ROOT_K]
        flagged(ix, "roster: ")
    ix = _copy(base)  # a tile's run record where the tile spans two runs
    t = int(np.nonzero(ix["trun"][:, 0] < 0)[0][0])
    ix["trun"][t] = (32 * t, 0)
    flagged(ix, "trun: ")
    ix = _copy(base)  # a non-finite record's tile without its flag
    t = int(np.nonzero(ix["tiles"]["nonfinite"])[0][0])
    ix["tiles"]["nonfinite"][t] = 0
    flagged(ix, "nonfinite flag")
    ix = _copy(base)  # a bound that bounds nothing
    ix["tiles"]["pr"][_finite_tile(ix)] += F(1e-3)
    flagged(ix, "pr wider")


# ------------------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def _planner(rec, max_batch=256, goal=(40.0, 0.0, 0.0, 0.0)):
    import clrrt
    from clrrt import abi
    pl = clrrt.Planner(clrrt.default_params(goal=goal, collision_mode=abi.CLRRT_COLLISION_STUB), max_nodes=1 << 13,
                       max_rows=1 << 16, max_batch=max_batch)
    pl.tree_load(wc.nodes_raw(rec))
    pl.set_option("nn_walk_min", 0)
    return pl


class _Main:
    """The main tree on the device with what the tests share: its index, the samples, the exact keys and the
    feasibility of every (sample, node) pair."""

    def __init__(self):
        from clrrt import abi
        self.rec, self.groups = wc.main_tree()
        self.pl = _planner(self.rec)
        self.feas_len = 2.1 * self.pl.params.ref_res
        self.sx, self.sy, self.ex, self.names = wc.samples(self.rec, self.groups, self.feas_len)
        self.ix = self.pl.walk_index()
        N, B = wc.N_MAIN, self.sx.size
        r = self.rec
        S = np.repeat(np.stack([self.sx, self.sy], axis=1), N, axis=0)
        tile = lambda v: np.tile(np.asarray(v, np.float64), B)  # noqa: E731
        keys = self.pl.selftest_units(abi.UNIT_DUBINS, np.column_stack([S, tile(r["x"]), tile(r["y"]), tile(r["h"]),
                                                                        tile(r["ce"])]))
        self.key = np.where(self.ex[:, None] != 0, keys[:, 0].reshape(B, N), keys[:, 1].reshape(B, N))
        fe = self.pl.selftest_units(abi.UNIT_FEASIBLE, np.column_stack(
            [S, tile(r["fx"]), tile(r["fy"]), tile(r["bx"]), tile(r["by"]), np.full(B * N, self.pl.params.ref_res)]))
        self.feasible = fe[:, 1].reshape(B, N) != 0  # as the searches decide it


@pytest.fixture(scope="module")
def main():
    m = _Main()
    yield m
    m.pl.close()


def _assert_index(ix, rec, what):
    stats = {}
    bad = check_index(ix, rec, stats)
    print(f"{what}: largest excess over the non-vacuity limits (<= 0 passes) {stats}")
    assert bad == [], bad
    return stats


@gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_main_tree_index(main, fused):
    ix = main.ix if not fused else main.pl.walk_index(fused=True)
    assert (ix["npad"], ix["ntiles"], ix["nsup"]) == (3072, 96, 3)
    st = _assert_index(ix, main.rec, f"main tree, fused {fused}")
    # the cases the tree is for are there
    assert st["tiles"]["nonfinite"] >= 1 and st["tiles"]["empty"] >= 1
    # (heading arcs past the "unbounded" limit; the place order starts with the ang_par sector, so no tile here spans
    # the ang_par circle: test_small_tree_index's 32-node tree has that tile)
    assert st["tiles"]["unbounded_th"] >= 1 and st["supers"]["unbounded_th"] >= 1
    head = ix["HEAD"] & ~ROOT_BIT
    runlen = np.bincount(head[:ix["count"]], minlength=ix["npad"])
    assert (ix["trun"][:, 0] >= 0).sum() >= 8 and runlen.max() > 64
    if not fused:
        assert ix["roster"][0] == ROOT_K and (ix["HEAD"] & ROOT_BIT).astype(bool).sum() == 1 + wc.ROOT_COPIES


@gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_range_index(main, fused):
    """Nodes [777, 777 + 1500): the range builder of clrrt_nn_range / the appended-node builder; no roster, no root
    marks, node ids kept."""
    ix = main.pl.walk_index(777, 1500, fused=bool(fused))
    _assert_index(ix, main.rec, f"range [777, 2277), fused {fused}")


@gpu
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("n", wc.SMALL_SIZES)
def test_small_tree_index(n, fused):
    rec = wc.small_tree(n)
    pl = _planner(rec)
    try:
        ix = pl.walk_index(fused=bool(fused))
        st = _assert_index(ix, rec, f"{n} nodes, fused {fused}")
        assert ix["npad"] == (n + 1023) // 1024 * 1024
        if n == 32:  # balanced arcs: the "no mean direction" branch
            assert ix["tiles"]["thh"][0] == 4 and ix["tiles"]["aph"][0] == 4
        if n >= 1023:
            head = ix["HEAD"] & ~ROOT_BIT
            assert np.bincount(head[:n]).max() >= (40 if fused else 80)  # the run of 80 (cut once at most when fused)
    finally:
        pl.close()


@gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_far_frame_index(fused):
    """A 2 km frame: float coordinates err by more than the discs' fixed margin, so the discs hold the exact positions
    only through the frame slack the builder is given."""
    rec = wc.far_tree()
    pl = _planner(rec, goal=wc.FAR_GOAL)
    try:
        ix = pl.walk_index(fused=bool(fused))
        assert frame_extent(ix) > 2000 and ix["slack"] > 1e-3
        _assert_index(ix, rec, f"far frame, fused {fused}")
        assert ((ix["tiles"]["pr"] >= 0) & (ix["tiles"]["pr"] < 0.06 + 3 * ix["slack"])).sum() >= 10  # whole cluster tiles
    finally:
        pl.close()


@gpu
def test_index_hook_errors(main):
    import clrrt
    pl = _planner(wc.small_tree(33), max_batch=64)
    try:
        pl.set_option("nn_walk_min", 8192)
        for fused in (False, True):
            with pytest.raises(clrrt.ClrrtError) as e:
                pl.walk_index(fused=fused)
            assert int(re.search(r"-> (-?\d+)", str(e.value)).group(1)) == ESTATE
    finally:
        pl.close()
    pl = _planner(main.rec, max_batch=64)  # the appended-node set holds 6 * 64 + 1024 nodes
    try:
        with pytest.raises(clrrt.ClrrtError) as e:
            pl.walk_index(fused=True)
        assert int(re.search(r"-> (-?\d+)", str(e.value)).group(1)) == ECAPACITY
        assert pl.walk_index(100, 1408, fused=True)["count"] == 1408
    finally:
        pl.close()


def _walk_one_inputs(m):
    """rsx, rsy, flen_t, dsR as walk_one forms them (clrrt_nnwalk.hip, the head of walk_one) -- restated, in float32."""
    ix = m.ix
    dl = F(ix["delta"])
    rsx, rsy = (m.sx - ix["ox"]).astype(F), (m.sy - ix["oy"]).astype(F)
    flen_t = F(m.feas_len) * (F(1) - F(1e-5)) - F(4) * dl
    Rx, Ry = F(ix["R"][0]), F(ix["R"][1])
    dsR = np.sqrt((rsx - Rx) * (rsx - Rx) + (rsy - Ry) * (rsy - Ry)) * (F(1) - F(1e-5)) - F(2) * dl - F(1e-4)
    assert dsR.dtype == F and rsx.dtype == F
    return rsx, rsy, F(flen_t), dsR, dl


@gpu
@pytest.mark.parametrize("which", ["tiles", "supers"])
def test_walk_lb_bounds_the_exact_keys(main, which):
    """Every (sample, tile) and (sample, super-tile) pair of the main tree: walk_lb on the device, given the downloaded
    record, against the smallest exact key of the tile's finite feasible members.  No tolerance."""
    ix = main.ix
    W = ix[which]
    size = 32 if which == "tiles" else 1024
    T, B = len(W), main.sx.size
    rsx, rsy, flen_t, dsR, _ = _walk_one_inputs(main)
    words = W.view(F).reshape(T, 16)
    cases = np.empty((B, T, 21), F)
    cases[:, :, :16] = words[None]
    cases[:, :, 16], cases[:, :, 17] = rsx[:, None], rsy[:, None]
    cases[:, :, 18], cases[:, :, 19], cases[:, :, 20] = main.ex[:, None], flen_t, dsR[:, None]
    out = main.pl.selftest_walk(2, cases.reshape(-1, 21)).astype(np.float64).reshape(B, T, 2)
    lb, lbd = out[:, :, 0], out[:, :, 1]
    assert not np.isnan(out).any()
    # the smallest key of each tile's finite feasible members
    m = _members(ix, main.rec)
    safe = np.where(m["valid"], m["id"], 0)
    ok = main.feasible[:, safe] & m["fin"][None, :]
    kmin = np.where(ok, main.key[:, safe], np.inf).reshape(B, T, size).min(axis=2)
    nonf = (W["nonfinite"] != 0)[None, :]
    with np.errstate(invalid="ignore"):  # (inf - inf where both are infinite: masked)
        gap = np.where(np.isfinite(kmin) & np.isfinite(lb), kmin - lb, np.inf)
    print(f"{which}: {B * T} pairs; smallest key - bound {gap.min():.6g}; bound +inf at {(lb == np.inf).sum()}, "
          f"-inf at {(lb == -np.inf).sum()}")
    bad = np.argwhere(lb > kmin)
    assert bad.size == 0, f"walk_lb above a member's key at (sample, {which}) {bad[:5]}: {lb[tuple(bad[0])]} > {kmin[tuple(bad[0])]}"
    bad = np.argwhere((lb == np.inf) & np.isfinite(kmin))
    assert bad.size == 0, f"walk_lb = +inf over a feasible member at {bad[:5]}"
    assert not ((lb == -np.inf) & ~nonf).any()
    assert (lbd <= lb).all()
    if which == "tiles":
        # circle floor: a bound of at least the code's 14.9f that the distance does not give (explore: no cost terms)
        D = np.hypot(rsx[:, None].astype(np.float64) - W["pcx"][None], rsy[:, None].astype(np.float64) - W["pcy"][None])
        floor = (main.ex[:, None] != 0) & np.isfinite(lb) & (lb >= F(14.9)) & (D - W["pr"][None] < 14.8)
        abeam = floor[main.names == "abeam"].any(axis=1).sum()
        inside = (D <= W["pr"][None]) & (W["pr"][None] >= 0)
        print(f"circle floor at {floor.sum()} explore pairs, {abeam} abeam samples; sample inside a tile disc at "
              f"{inside.sum()} pairs")
        assert abeam >= 1
        assert inside[main.names == "tile_centre"].any()


def _t2(tx, ty):
    """walk_key_range's t2 as it forms it (float32, no contraction) -- restated."""
    tx, ty = tx.astype(F), ty.astype(F)
    return tx * tx + ty * (ty - F(2) * F(4.77))


def _key_range_cases():
    rng = np.random.default_rng(31)
    n = 200_000
    scale = np.exp(rng.uniform(np.log(0.05), np.log(40.0), n))
    a = rng.uniform(0, np.pi, n)
    tx, ty = scale * np.cos(a), scale * np.sin(a)
    q = n // 4  # a quarter on the turning circle: |t2| < 0.02 about the centre (0, rho)
    t2 = rng.uniform(-0.02, 0.02, q)
    t2[:7] = (-0.02, -0.01, -1e-3, 0.0, 1e-3, 0.01, 0.02)
    dc = np.sqrt(4.77 ** 2 + t2)
    b = rng.uniform(-np.pi, np.pi, q)
    tx[:q], ty[:q] = dc * np.cos(b), np.abs(4.77 + dc * np.sin(b))
    pos_err = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), n))
    return tx.astype(F), ty.astype(F), pos_err.astype(F)


@gpu
@pytest.mark.parametrize("fn", [0, 1])
def test_walk_key_range_brackets_the_key(main, fn):
    """2e5 offsets (tx, ty >= 0, pos_err): lo <= key <= hi for the key of four offsets within pos_err of the given one
    (the sample (tx + jx, ty + jy) from a node at the origin with heading 0: its rotated float offset is the float
    sample itself; a jitter whose float offset would leave the pos_err disc is dropped for that case)."""
    from clrrt import abi
    tx, ty, pe = _key_range_cases()
    out = main.pl.selftest_walk(fn, np.column_stack([tx, ty, pe])).astype(np.float64)
    lo, hi = out[:, 0], out[:, 1]
    assert not np.isnan(out).any()
    t2 = _t2(tx, ty)
    assert (np.abs(t2[:len(t2) // 4]) < 0.021).all()
    assert np.isfinite(lo[t2 >= F(0.01)]).all() and np.isfinite(hi[t2 >= F(0.01)]).all()
    assert (lo[t2 <= F(-0.01)] >= F(14.9)).all()  # (the code's 14.9f)
    rng = np.random.default_rng(32)
    n = tx.size
    worst_lo = worst_hi = np.inf
    for j in range(4):
        r = pe.astype(np.float64) * (1.0 if j < 2 else np.sqrt(rng.uniform(0, 1, n)))
        a = rng.uniform(-np.pi, np.pi, n)
        jx, jy = (tx.astype(np.float64) + r * np.cos(a)).astype(F), (ty.astype(np.float64) + r * np.sin(a)).astype(F)
        inside = np.hypot(jx.astype(np.float64) - tx, np.abs(jy).astype(np.float64) - ty) <= pe
        jx, jy = np.where(inside, jx, tx), np.where(inside, jy, ty)
        z = np.zeros(n)
        key = main.pl.selftest_units(abi.UNIT_DUBINS, np.column_stack([jx, jy, z, z, z, z]))[:, 0]
        assert np.isfinite(key).all()
        worst_lo, worst_hi = min(worst_lo, (key - lo).min()), min(worst_hi, (hi - key).min())
        bad = np.nonzero((lo > key) | (key > hi))[0]
        assert bad.size == 0, (f"fn {fn}, jitter {j}: {bad.size} keys outside [lo, hi], e.g. case {bad[0]}: tx {tx[bad[0]]} "
                               f"ty {ty[bad[0]]} pos_err {pe[bad[0]]}: {lo[bad[0]]} <= {key[bad[0]]} <= {hi[bad[0]]}")
    print(f"fn {fn}: smallest key - lo {worst_lo:.3g}, hi - key {worst_hi:.3g}; jittered onto the disc's rim and inside")


@gpu
def test_stage1_margins_on_the_main_tree(main):
    """Every (sample, record) pair of the main tree through stage 1's composite margins -- restated from walk_one's
    stage1, not called: the offset rotated in float from the frame records, pos_err = 4 dl + 1e-6 (|tx| + ty), the
    cost added and both bounds widened by 1e-6 relative -- around walk_key_range on the device."""
    ix = main.ix
    rsx, rsy, _, _, dl = _walk_one_inputs(main)
    n = ix["count"]
    m = _members(ix, main.rec)
    P, CE, ids = ix["P"][:n], ix["CE"][:n], ix["ID"][:n]
    fin = m["fin"][:n]
    qx, qy = rsx[:, None] - P[None, :, 0], rsy[:, None] - P[None, :, 1]
    tx = P[None, :, 2] * qx - P[None, :, 3] * qy
    ty = np.abs(P[None, :, 3] * qx + P[None, :, 2] * qy)
    pe = F(4) * dl + F(1e-6) * (np.abs(tx) + ty)
    assert tx.dtype == F and pe.dtype == F
    worst = {}
    for fn in (0, 1):
        out = main.pl.selftest_walk(fn, np.stack([tx, ty, pe], axis=2).reshape(-1, 3)).reshape(tx.shape + (2,))
        cst = np.where(main.ex[:, None] != 0, F(0), CE[None, :]).astype(F)
        tlo, thi = cst + out[:, :, 0], cst + out[:, :, 1]
        with np.errstate(invalid="ignore"):  # (infinite bounds and the non-finite records' NaN: masked by ok)
            lbt, ubt = tlo - F(1e-6) * np.abs(tlo), thi + F(1e-6) * np.abs(thi)
        key = main.key[:, ids]
        ok = fin[None, :] & np.isfinite(key)
        assert ok.sum() > 0.99 * ok.size
        bad = np.argwhere(ok & ((lbt.astype(np.float64) > key) | (key > ubt.astype(np.float64))))
        assert bad.size == 0, f"fn {fn}: key outside stage 1's bounds at (sample, place) {bad[:5]}"
        with np.errstate(invalid="ignore"):
            worst[fn] = (np.where(ok, key - lbt, np.inf).min(), np.where(ok, ubt - key, np.inf).min())
    print(f"stage 1: smallest (key - lbt, ubt - key) per fn {worst}")


@gpu
def test_acos_atan2_apx_errors(main):
    """acos_apx within 7e-5 rad and atan2_apx within 1e-6 rad of float64 numpy, as the code comments claim."""
    rng = np.random.default_rng(33)
    n = 2_000_000
    x = rng.uniform(-1, 1, n).astype(F)
    y = rng.uniform(-1, 1, n).astype(F)
    s = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)).astype(F)
    edge = np.array([(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (0.5, 0.5), (-0.25, 0.25),
                     (1e-30, 1), (1, 1e-30), (-1e-30, -1)], F)
    k = len(edge)
    y[:k], x[:k], s[:k] = edge[:, 0], edge[:, 1], 1
    near = slice(k, k + 100_000)  # close to the ends of acos's range and to |x| = |y|
    x[near] = np.where(rng.uniform(0, 1, 100_000) < 0.5, 1, -1) * (1 - np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), 100_000)))
    y[near] = x[near] * (1 + rng.uniform(-1e-6, 1e-6, 100_000))
    out = main.pl.selftest_walk(3, np.column_stack([y, x])).astype(np.float64)
    ea = np.abs(out[:, 0] - np.arccos(x.astype(np.float64)))
    print(f"acos_apx: largest error {ea.max():.3g} rad at x = {x[ea.argmax()]}")
    assert ea.max() <= 7e-5
    ys, xs = (y * s).astype(F), (x * s).astype(F)  # atan2 over six decades of scale
    nz = (ys != 0) | (xs != 0)
    out = main.pl.selftest_walk(3, np.column_stack([ys, xs])).astype(np.float64)
    et = np.abs(out[:, 1] - np.arctan2(ys.astype(np.float64), xs.astype(np.float64)))[nz]
    print(f"atan2_apx: largest error {et.max():.3g} rad")
    assert et.max() <= 1e-6


@gpu
def test_bound_codes(main):
    """lc_dec is non-decreasing; lc_enc(b) is the largest code that decodes to <= b (by the device's own lc_dec values);
    lc_le agrees with it for finite thresholds."""
    codes = np.arange(256)
    dec = main.pl.selftest_walk(4, np.column_stack([np.zeros(256), codes]))[:, 2].astype(np.float64)
    assert dec[0] == -np.inf and dec[255] == np.inf and np.isfinite(dec[1:255]).all()
    assert (np.diff(dec) >= 0).all() and (np.diff(dec[1:255]) > 0).all()
    rng = np.random.default_rng(34)
    b = np.exp2(rng.uniform(-6, 13, 100_000)).astype(F)
    b = np.concatenate([b, dec[1:255].astype(F), np.nextafter(dec[1:255].astype(F), F(0)),
                        np.array([0, -0.0, -1, -1e30, np.inf, -np.inf, np.nan, 1e-30, 3e38], F)])
    out = main.pl.selftest_walk(4, np.column_stack([b, np.zeros_like(b)]))
    enc, le = out[:, 0].astype(np.int64), out[:, 1].astype(np.int64)
    assert ((enc >= 0) & (enc <= 255)).all()
    bd = b.astype(np.float64)
    num = ~np.isnan(bd)
    assert (dec[enc][num] <= bd[num]).all()
    below = num & (enc < 254)
    assert (bd[below] < dec[enc[below] + 1]).all()
    assert (enc[np.isnan(bd)] == 0).all() and (enc[bd == np.inf] == 255).all() and (enc[bd < dec[1]] == 0).all()
    fin = np.isfinite(bd)
    assert (le[fin] == enc[fin]).all() and (le[bd == np.inf] == 255).all()
    assert set(np.unique(enc[:100_000])) >= set(range(1, 255))  # every finite code is reached


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


STRATEGIES = ["walk", "walk_stateless", "walk_coded", "walk_split", "walk_split_coded", "walk_persistent",
              "walk_coded_persistent"]


@pytest.fixture(scope="module")
def brute_lists(main):
    from nn_strategies import nn_strategy
    smp = wc.sample_structs(main.sx, main.sy, main.ex)
    nn_strategy(main.pl, "brute")
    try:
        return smp, main.pl.sort_nodes_batch(smp, exact=False)
    finally:
        main.pl.set_option("nn_walk_min", 0)


@gpu
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_lists_on_the_adversarial_tree(main, brute_lists, strategy):
    """Every walk strategy (float state, fp16 stateless, coded bytes, overflow split, persistent grid) returns the brute
    force's ids and key bits for all 256 samples."""
    from nn_strategies import nn_strategy
    smp, (ib, kb) = brute_lists
    assert (ib >= 0).any(axis=1).sum() > 200
    nn_strategy(main.pl, strategy)
    try:
        iw, kw = main.pl.sort_nodes_batch(smp, exact=False)
    finally:
        nn_strategy(main.pl, "walk")
    bad = np.nonzero((ib != iw).any(axis=1) | (_bits(kb) != _bits(kw)).any(axis=1))[0]
    assert bad.size == 0, (f"{strategy}: samples {bad[:8]} ({main.names[bad[:8]]}) differ, e.g. {ib[bad[0]]} {kb[bad[0]]} "
                           f"vs {iw[bad[0]]} {kw[bad[0]]}")


@gpu
def test_lists_equal_the_oracle(main, brute_lists):
    """32 samples, every boundary kind among them, against the CPU oracle's sort_nodes(stable) on the tree with the
    NaN-key record made keyed-but-infeasible (walk_cases.finite_for_oracle): ids and key bits.

    Not the samples on a node's position: there the reference's float formula gives that node (and every record of its
    run) a NaN key -- (5 rho^2 - df^2) / (4 rho^2) rounds to 1.0000001 and acosf returns NaN -- and std::stable_sort
    over a NaN key has no defined order, so the oracle's list is not a reference for them.  The engine keeps NaN keys
    out of every list; for those samples that, and the brute force's lists (test_lists_on_the_adversarial_tree), are
    what is checked."""
    from clrrt import abi
    from nn_strategies import nn_strategy
    from oracle_binding import Oracle
    rec2 = wc.finite_for_oracle(main.rec, main.groups)
    pick = []
    nan_key = np.isnan(np.delete(main.key, np.nonzero(np.isnan(main.rec["x"]))[0], axis=1)).any(axis=1)
    assert set(main.names[nan_key]) == {"on_node"} and nan_key.sum() == 8
    smp_all, (ib, _) = brute_lists
    for q in np.nonzero(nan_key)[0]:  # the NaN-key records are in no list
        listed = ib[q][ib[q] >= 0]
        assert listed.size > 0 and not np.isnan(main.key[q, listed]).any()
    for name in ("tile_centre", "on_ref_back", "circle", "abeam", "feas_len", "cone_edge"):
        at = np.nonzero(main.names == name)[0]
        pick += list(at[:: max(1, at.size // 4)][:4])
    pick += list(np.nonzero(main.names == "uniform")[0][:32 - len(pick)])
    assert len(pick) == 32
    o = Oracle(abi.default_params(collision_mode=abi.CLRRT_COLLISION_STUB), None)
    o.load_tree(wc.nodes_raw(rec2))
    pl = _planner(rec2)
    try:
        nn_strategy(pl, "walk")
        smp = wc.sample_structs(main.sx[pick], main.sy[pick], main.ex[pick])
        iw, kw = pl.sort_nodes_batch(smp, exact=False)
        for q, s in enumerate(smp):
            ids, keys = o.sort_nodes(s.x, s.y, s.explore, stable=True)
            k = min(len(ids), 10)
            assert list(iw[q][:k]) == ids[:k] and (iw[q][k:] == -1).all(), (pick[q], main.names[pick[q]], ids, iw[q])
            assert np.array_equal(_bits(kw[q][:k]), _bits(keys[:k])), (pick[q], keys, kw[q])
    finally:
        pl.close()
