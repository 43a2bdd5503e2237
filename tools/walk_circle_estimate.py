"""What the circle floor removes from the walk search's admissible tiles (CPU oracle + numpy; clrrt_nnwalk.hip walk_lb).
Grows the cfg3 scene by BATCH rounds (seed 31, 16384 samples per round, defer_steps 128), orders the nodes as the
kind-5 / hscale-50 index does (k_walk_keys: ang_par sector, 3D Morton code of x, y and 0.5 rho * heading, coarse
ref.back() cell; the frame box here is the nodes' and samples' bounding box + 1 m, which sets the order's grain only),
forms the tiles' bounds as walk_tile_bounds does (float32) and, for fresh explore samples (kth = the 11th smallest key
among the feasible records, keys and feasibleNode restated in numpy and checked against the oracle's own list of 10),
counts the tiles with walk_lb <= kth -- without and with the circle floor -- for tiles of 32, 16 and 8 records.  Also:
tiles holding a member of the oracle's list that the floor cuts (must be 0), and how many admissible tiles hold a key
<= kth / a feasible record at all (an estimate, not the oracle).
Usage: python tools/walk_circle_estimate.py [rounds [samples]] > profiles/<name>.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clrrt import abi, scenes  # noqa: E402
from oracle_binding import Oracle  # noqa: E402
from test_nnwalk_bounds import dubins_key_f32  # noqa: E402

F = np.float32
RHO = F(4.77)
PI = F(3.14159265)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n_smp = int(sys.argv[2]) if len(sys.argv) > 2 else 600
B = 16384
params = abi.default_params(collision_mode=abi.CLRRT_COLLISION_OBB)
o = Oracle(params, scenes.urban_scene(200))
Oracle.srand(31)
o.init_tree()
o.expand_batch(rounds * B, B, stable=True, defer_steps=128, threads=min(32, os.cpu_count() or 4))
t = o.nodes()
N = len(t["parent"])
st, ce, rb, ap = t["state"], t["costE"].astype(F), t["ref_back"], t["ang_par"]
xy, ex = o.draw_samples(n_smp)
print(f"cfg3 scene, seed 31, B = {B}, defer_steps 128, {rounds} rounds: {N} nodes; {int((ex == 1).sum())} explore "
      f"samples of {n_smp}")


def spread3(v):
    x = v.astype(np.uint64) & np.uint64(0xffff)
    for sh, m in ((16, 0x0000ff0000ff), (8, 0x00f00f00f00f), (4, 0x0c30c30c30c3), (2, 0x249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(m)
    return x


def spread(v):
    x = v.astype(np.uint64) & np.uint64(0xffff)
    for sh, m in ((8, 0x00ff00ff), (4, 0x0f0f0f0f), (2, 0x33333333), (1, 0x55555555)):
        x = (x | (x << np.uint64(sh))) & np.uint64(m)
    return x


# the index order (k_walk_keys, kind 5)
x0, y0 = min(st[:, 0].min(), xy[:, 0].min()) - 1.0, min(st[:, 1].min(), xy[:, 1].min()) - 1.0
x1, y1 = max(st[:, 0].max(), xy[:, 0].max()) + 1.0, max(st[:, 1].max(), xy[:, 1].max()) + 1.0
hrho = 4.77 * 0.5
scale = 65535.0 / max(x1 - x0, y1 - y0, 2 * np.pi * hrho)
c, s = np.cos(-st[:, 2]).astype(F), np.sin(-st[:, 2]).astype(F)  # the records' (cos, sin)(-heading)
ca, sa = np.cos(ap).astype(F), np.sin(ap).astype(F)
apf = ap.astype(F)
sector = np.clip(np.floor((apf + PI) * F(8 / 6.2831853)).astype(np.int64), 0, 7).astype(np.uint64)
ang = np.arctan2(-s, c).astype(np.float64)
ang = ang - 2 * np.pi * np.floor((ang + np.pi) / (2 * np.pi))
q = lambda v: np.clip(v, 0.0, 65535.0).astype(np.uint64)  # noqa: E731
m3 = spread3(q((st[:, 0] - x0) * scale)) | (spread3(q((st[:, 1] - y0) * scale)) << np.uint64(1)) | \
    (spread3(q((ang + np.pi) * hrho * scale)) << np.uint64(2))
low = (spread(q((rb[:, 0] - x0) * scale) >> np.uint64(9)) |
       (spread(q((rb[:, 1] - y0) * scale) >> np.uint64(10)) << np.uint64(1))) & np.uint64(0x1fff)
key = (sector << np.uint64(61)) | (m3 << np.uint64(13)) | low
order = np.argsort(key, kind="stable")

# float frame records (k_walk_gather) and the frame's slack
ox, oy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
slack = F((max(x1 - x0, y1 - y0) + 1.0) * 2.0 ** -24)
PX, PY = (st[order, 0] - ox).astype(F), (st[order, 1] - oy).astype(F)
QX, QY = (rb[order, 0] - ox).astype(F), (rb[order, 1] - oy).astype(F)
PC, PS, QC, QS, CE = c[order], s[order], ca[order], sa[order], ce[order]


def acos_apx(x):
    ax = np.minimum(np.abs(x), F(1))
    r = np.sqrt(F(1) - ax) * (F(1.5707288) + ax * (F(-0.2121144) + ax * (F(0.0742610) + ax * F(-0.0187293))))
    return np.where(x < 0, PI - r, r).astype(F)


def tile_bounds(size):
    """walk_tile_bounds for tiles of `size` records (the last tile padded by repeating its last record)."""
    nt = -(-N // size)
    idx = np.minimum(np.arange(nt * size), N - 1).reshape(nt, size)
    px, py, qx, qy = PX[idx], PY[idx], QX[idx], QY[idx]
    w = {}
    w["pcx"], w["pcy"] = px.mean(1, dtype=F), py.mean(1, dtype=F)
    w["rcx"], w["rcy"] = qx.mean(1, dtype=F), qy.mean(1, dtype=F)
    ux, uy = PC[idx].sum(1, dtype=F), (-PS[idx]).sum(1, dtype=F)
    ax, ay = QC[idx].sum(1, dtype=F), QS[idx].sum(1, dtype=F)
    un, an = np.sqrt(ux * ux + uy * uy), np.sqrt(ax * ax + ay * ay)
    uok, aok = un > F(1e-3) * size, an > F(1e-3) * size
    with np.errstate(all="ignore"):
        ux, uy = np.where(uok, ux / un, F(1)), np.where(uok, uy / un, F(0))
        ax, ay = np.where(aok, ax / an, F(1)), np.where(aok, ay / an, F(0))
    dp = np.sqrt((px - w["pcx"][:, None]) ** 2 + (py - w["pcy"][:, None]) ** 2)
    dr = np.sqrt((qx - w["rcx"][:, None]) ** 2 + (qy - w["rcy"][:, None]) ** 2)
    ud = ((PC[idx] * ux[:, None] - PS[idx] * uy[:, None]) / np.sqrt(PC[idx] ** 2 + PS[idx] ** 2)).min(1)
    ad = ((QC[idx] * ax[:, None] + QS[idx] * ay[:, None]) / np.sqrt(QC[idx] ** 2 + QS[idx] ** 2)).min(1)
    w["pr"] = dp.max(1) * F(1 + 1e-5) + F(2) * slack + F(1e-5)
    w["rr"] = dr.max(1) * F(1 + 1e-5) + F(2) * slack + F(1e-5)
    w["thx"], w["thy"] = ux, uy
    w["thh"] = np.where(uok, np.arccos(np.clip(ud, -1, 1)).astype(F) + F(2e-3), F(4))
    w["apx"], w["apy"] = ax, ay
    w["aph"] = np.where(aok, np.arccos(np.clip(ad, -1, 1)).astype(F) + F(2e-3), F(4))
    return {k: v.astype(F) for k, v in w.items()}, idx


def walk_lb(w, sx, sy, flen, floor):
    """walk_lb for an explore sample at frame point (sx, sy); floor: with the circle floor."""
    with np.errstate(all="ignore"):
        ex2, ey2 = sx - w["rcx"], sy - w["rcy"]
        E2 = np.sqrt(ex2 * ex2 + ey2 * ey2)
        inf = E2 + w["rr"] < flen
        iE = F(1) / E2
        a2 = F(1.57079633) - acos_apx(w["rr"] * iE)
        ang2 = acos_apx((ex2 * w["apx"] + ey2 * w["apy"]) * iE)
        inf |= (E2 > w["rr"]) & (w["aph"] < 3) & (ang2 - a2 - w["aph"] > F(0.78539816 + 5e-3))
        dx, dy = sx - w["pcx"], sy - w["pcy"]
        D = np.sqrt(dx * dx + dy * dy)
        lb = D - w["pr"]
        arc = (D > w["pr"]) & (w["thh"] < 3)
        iD = F(1) / D
        A = (F(1.57079633) - acos_apx(w["pr"] * iD)) + w["thh"] + F(3e-3)
        an = acos_apx((dx * w["thx"] + dy * w["thy"]) * iD)
        lb = np.where(arc, np.maximum(lb, RHO * (an - A)), lb)
        z = np.minimum(an, PI - an) - A
        z2 = z * z
        g = (F(2) * RHO) * (z + z * z2 * (F(-1) / F(6) + z2 * (F(1) / F(120) - z2 * (F(1) / F(5040)))))
        d0, d1 = D - w["pr"], D + w["pr"]
        circ = arc & (z > 0) & (np.maximum(d0 * (d0 - g), d1 * (d1 - g)) <= F(-0.011))
        lb = lb - F(2e-3) - F(1e-5) * np.abs(lb)
        if floor:
            lb = np.where(circ, np.maximum(lb, F(14.9)), lb)
    return np.where(inf, np.inf, lb)


flen = F(2.1 * params.ref_res)


def feasible(sx, sy, r):
    vx, vy = sx - QX[r], sy - QY[r]
    dot, vv = vx * QC[r] + vy * QS[r], vx * vx + vy * vy
    return (vv >= flen * flen) & (dot > 0) & (dot * dot >= F(0.5) * vv)


def keys_of(sx, sy, r):
    qx, qy = sx - PX[r], sy - PY[r]
    return dubins_key_f32(PC[r] * qx - PS[r] * qy, PS[r] * qx + PC[r] * qy)


ALL = np.arange(N)


def kth_of(sx, sy, okeys):
    """The 11th smallest key among the feasible records (the oracle lists sort_limit = 10; its last key must not
    exceed it)."""
    k = keys_of(sx, sy, ALL)[feasible(sx, sy, ALL)]
    k = k[np.isfinite(k)]
    if len(k) < 11 or len(okeys) < 10:
        return np.inf
    kth = np.partition(k, 10)[10]
    assert kth >= okeys[-1] - 1e-3, (kth, okeys[-1])
    return F(kth)


sel = np.nonzero(ex == 1)[0]
place = np.empty(N, dtype=np.int64)
place[order] = np.arange(N)
for size in (32, 16, 8):
    w, idx = tile_bounds(size)
    sup, _ = tile_bounds(size * 32)
    adm = {False: [], True: []}
    cut_members = fired = with_key = with_feas = n_list = 0
    for j in sel:
        ids, keys = o.sort_nodes(xy[j, 0], xy[j, 1], 1, stable=True)
        sx, sy = F(xy[j, 0] - ox), F(xy[j, 1] - oy)
        kth = kth_of(sx, sy, keys)
        if not np.isfinite(kth):
            continue  # no 11th key: every tile is admissible under either bound
        n_list += 1
        lbs = {}
        for floor in (False, True):
            lb = np.maximum(walk_lb(w, sx, sy, flen, floor), np.repeat(walk_lb(sup, sx, sy, flen, floor), 32)[:len(w["pr"])])
            lbs[floor] = lb
            adm[floor].append(int((lb <= kth).sum()))
        fired += int(((lbs[True] > kth) & (lbs[False] <= kth)).sum())
        mt = place[np.array(ids[:11])] // size
        cut_members += int((lbs[True][mt] > kth).sum())
        if size == 32:  # what the admissible tiles hold (numpy keys and feasibleNode)
            a = np.nonzero(lbs[True] <= kth)[0]
            r = idx[a]
            with_key += int((keys_of(sx, sy, r) <= kth).any(1).sum())
            with_feas += int(feasible(sx, sy, r).any(1).sum())
    a0, a1 = np.mean(adm[False]), np.mean(adm[True])
    print(f"tiles of {size:2d} records ({len(w['pr'])} tiles), {n_list} explore samples with an 11th key: admissible tiles "
          f"per sample {a0:.1f} -> {a1:.1f} with the circle floor ({(a1 / a0 - 1):+.1%}; {fired / n_list:.1f} cut per "
          f"sample); tiles holding a list member cut: {cut_members} of {n_list} x {len(w['pr'])}")
    if size == 32:
        print(f"   of the {a1:.1f} admissible tiles per sample {with_key / n_list:.1f} hold a key <= kth and "
              f"{with_feas / n_list:.1f} a feasible record")
    sys.stdout.flush()
