"""Obstacle scenes and vehicle states for tests/test_collision_cull.py (fixed seeds, no fixtures).

An obstacle is (cx, cy, theta, size_x, size_y, vx, vy); a state is 10 doubles with x, y, heading in columns
0..2 and the time in column 6.  The vehicle box of checkObsDistance is centred 1.424 m ahead of the state's
position along its heading (old_collisioncheck.cpp:34-36), 4.848 x 2 m: half-diagonal VEH_RAD, and a corner
leads when the heading is CORNER off the approach direction.
"""
import numpy as np

from clrrt import scenes
from clrrt.scenes import _Lcg

VEH_RAD = float(np.hypot(2.424, 1.0))
CORNER = float(np.arctan2(1.0, 2.424))
OFFSETS = (4096.0, 2.0 ** 14, 2.0 ** 17, 2.0 ** 18, 2.0 ** 20, 2.0 ** 22)
EXEMPT_BOUND = 2.0 ** 15  # CULL_EXEMPT_BOUND (clrrt_internal.hpp): obstacles reaching past it are never culled


def _urban_box(g):
    return g.u(-3.14, 3.14), g.u(2.0, 6.0), g.u(4.0, 10.0)


def _stack(n=100):
    g = _Lcg(77)
    out = []
    for _ in range(n):
        x, y = 22.0 + g.u(-0.5, 0.5), 5.0 + g.u(-0.5, 0.5)
        out.append((x, y, *_urban_box(g), 0.0, 0.0))
    return np.asarray(out, dtype=np.float64)


def _every(obs, k, first, vmax, seed):
    """Obstacles first, first + k, ... get a (non-zero) velocity: moving ids interleave with static ones."""
    g = _Lcg(seed)
    obs = obs.copy()
    for j in range(first, len(obs), k):
        obs[j, 5] = g.u(0.1, vmax) * (1 if j % 2 else -1)
        obs[j, 6] = g.u(-vmax, vmax)
    return obs


def _spread(n, seed):
    g = _Lcg(seed)
    out = []
    for _ in range(n):
        x, y = g.u(0.0, 600.0), g.u(-300.0, 300.0)
        out.append((x, y, *_urban_box(g), 0.0, 0.0))
    return np.asarray(out, dtype=np.float64)


_TRIPLE = np.asarray([(20.0, 3.0, 0.7, 4.4, 8.6, 0.0, 0.0),
                      (22.5, 5.0, -1.1, 3.0, 6.0, 0.0, 0.0),
                      (18.5, 6.5, 2.3, 5.2, 9.4, 0.0, 0.0)])


def scene(name):
    """(M, 7) obstacles of the named scene."""
    if name in ("single", "pair", "triple"):
        return _TRIPLE[:{"single": 1, "pair": 2, "triple": 3}[name]].copy()
    if name == "stack":
        return _stack()
    if name == "stack_mov":
        return _every(_stack(), 7, 3, 0.5, 5)
    if name == "urban60":
        return scenes.urban_scene(60)
    if name == "interleaved":
        return _every(scenes.urban_scene(60), 3, 1, 2.0, 9)
    if name == "all_moving":
        return scenes.urban_scene(0, 20)
    if name == "far_line":
        o = _TRIPLE[:2].copy()
        o[1, 0:2] = (3020.0, 3.0)
        return o
    if name == "far_L":
        o = _TRIPLE.copy()
        o[1, 0:2] = (3020.0, 3.0)
        o[2, 0:2] = (20.0, 3003.0)
        return o
    if name == "near_and_far":  # a grid near the origin, one static obstacle at 2^20 m beside it
        return np.concatenate([_TRIPLE, shifted(_TRIPLE[:1], 2.0 ** 20)])
    if name.startswith("capacity_"):
        return _spread(int(name.split("_")[1]), 31)
    raise KeyError(name)


def shifted(obs, off):
    """The scene moved by (off, -off)."""
    o = np.array(obs, dtype=np.float64)
    o[:, 0] += off
    o[:, 1] -= off
    return o


def _state(vx, vy, th, t):
    """States whose vehicle-box centre is (vx, vy)."""
    vx, vy, th, t = np.broadcast_arrays(np.asarray(vx, float), np.asarray(vy, float), np.asarray(th, float),
                                        np.asarray(t, float))
    s = np.zeros((vx.size, 10))
    s[:, 0] = vx.ravel() - 1.424 * np.cos(th.ravel())
    s[:, 1] = vy.ravel() - 1.424 * np.sin(th.ravel())
    s[:, 2] = th.ravel()
    s[:, 6] = t.ravel()
    return s


def uniform_states(obs, n, seed, tmax=10.0):
    """Half the poses uniform over the obstacles' bounding box plus 10 m, half within 6 m of an obstacle's
    position at the state's time (so that sparse scenes still collide), headings in (-pi, pi), times in (0, tmax)."""
    r = np.random.RandomState(seed)
    lo, hi = obs[:, 0:2].min(axis=0) - 10.0, obs[:, 0:2].max(axis=0) + 10.0
    m = n // 2
    t = r.uniform(0.0, tmax, n)
    th = r.uniform(-np.pi, np.pi, n)
    x = r.uniform(lo[0], hi[0], n)
    y = r.uniform(lo[1], hi[1], n)
    j = r.randint(0, len(obs), n - m)
    x[m:] = obs[j, 0] + obs[j, 5] * t[m:] + r.uniform(-6.0, 6.0, n - m)
    y[m:] = obs[j, 1] + obs[j, 6] * t[m:] + r.uniform(-6.0, 6.0, n - m)
    return _state(x, y, th, t)


def _f32_steps(v, k):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return float(v)


def grid_states(g, seed, nborders=24):
    """Poses outside the grid on each of its four sides, one at 3e9 m (the cell index leaves int range), and
    poses whose vehicle centre lies within +-2 float ulps of cell borders x0 + k / inv, y0 + k / inv and of the
    grid origin.  g: Planner.grid_info() of a scene with a grid."""
    assert g["gw"] > 0
    r = np.random.RandomState(seed)
    x0, y0, cs = float(g["x0"]), float(g["y0"]), 1.0 / float(g["inv"])
    w, h = g["gw"] * cs, g["gh"] * cs
    vx = [x0 - 3.0, x0 + w + 3.0, x0 + 0.5 * w, x0 + 0.5 * w, x0 - 0.01, x0 + w + 0.01, 3e9, x0 + 0.5 * w]
    vy = [y0 + 0.5 * h, y0 + 0.5 * h, y0 - 3.0, y0 + h + 3.0, y0 - 0.01, y0 + h + 0.01, y0 + 0.5 * h, -3e9]
    inv = np.float32(g["inv"])
    ks = [0, 1, g["gw"] - 1, g["gw"]] + list(r.randint(0, g["gw"] + 1, nborders))
    for k in ks:
        bx = np.float32(g["x0"]) + np.float32(k) / inv
        ky = int(r.randint(0, g["gh"] + 1)) if k else 0
        by = np.float32(g["y0"]) + np.float32(ky) / inv
        for d in (-2, -1, 0, 1, 2):
            vx.append(_f32_steps(bx, d)); vy.append(float(by) + (0.3 * cs if k else 0.0))
            vx.append(float(bx) + (0.3 * cs if k else 0.0)); vy.append(_f32_steps(by, d))
    n = len(vx)
    return _state(vx, vy, r.uniform(-np.pi, np.pi, n), r.uniform(0.0, 10.0, n))


def first_contact_states(oracle, obs, n, seed, tmax=0.0):
    """n attempts -> 2 n states: pick an obstacle, an approach direction and a heading (every third attempt presents
    a vehicle corner first: approach direction +- CORNER; every third a face), then bisect the distance of the
    vehicle centre from the obstacle centre between 0 and 40 m with the oracle until the bracket is below 1e-9 m.
    Returns the last colliding and the first free state of every attempt, and asserts every attempt brackets."""
    r = np.random.RandomState(seed)
    j = r.randint(0, len(obs), n)
    phi = r.uniform(-np.pi, np.pi, n)
    psi = r.uniform(-np.pi, np.pi, n)
    kind = np.arange(n) % 3
    psi = np.where(kind == 0, phi + np.where(r.rand(n) < 0.5, CORNER, -CORNER), psi)
    psi = np.where(kind == 1, phi + (np.arange(n) % 2) * (np.pi / 2), psi)
    t = r.uniform(0.0, tmax, n) if tmax > 0 else np.zeros(n)
    cx, cy = obs[j, 0] + obs[j, 5] * t, obs[j, 1] + obs[j, 6] * t

    def at(d):
        return _state(cx + d * np.cos(phi), cy + d * np.sin(phi), psi, t)

    lo, hi = np.zeros(n), np.full(n, 40.0)
    assert np.all(oracle.check_obs_n(at(lo))[0] == 0), "a vehicle centred on an obstacle must collide"
    assert np.all(oracle.check_obs_n(at(hi))[0] != 0), "a vehicle 40 m away must be free"
    while np.max(hi - lo) >= 1e-9:
        mid = 0.5 * (lo + hi)
        hit = oracle.check_obs_n(at(mid))[0] == 0
        lo = np.where(hit, mid, lo)
        hi = np.where(hit, hi, mid)
    return np.concatenate([at(lo), at(hi)])


def nonfinite_block(states):
    """A wave of 64 of the given states with one NaN and one +inf x among them."""
    b = np.array(states[:64], dtype=np.float64)
    assert len(b) == 64
    b[5, 0] = np.nan
    b[40, 0] = np.inf
    return b


def state_in_cell(g, cell, th=0.3, t=0.0):
    """A state whose vehicle centre is the middle of grid cell `cell`; cell -1: outside the grid."""
    x0, y0, cs = float(g["x0"]), float(g["y0"]), 1.0 / float(g["inv"])
    if cell < 0:
        return _state(x0 - 5.0, y0 - 5.0, th, t)[0]
    gx, gy = cell % g["gw"], cell // g["gw"]
    return _state(x0 + (gx + 0.5) * cs, y0 + (gy + 0.5) * cs, th, t)[0]


def cell_counts(g):
    """count -> a cell whose list has that many static obstacles (the cell nearest the grid's middle)."""
    cnt = np.diff(g["start"].astype(np.int64))
    out = {}
    for c in np.argsort(np.abs(np.arange(len(cnt)) - len(cnt) // 2), kind="stable"):
        out.setdefault(int(cnt[c]), int(c))
    return out


def lanes_for_total(counts, total, nlanes=64):
    """Fewest lane candidate counts (from `counts`, each >= 1) that sum to `total`; None when impossible."""
    coins = sorted(c for c in counts if c >= 1)
    best = {0: []}
    for s in range(1, total + 1):
        cand = [best[s - c] + [c] for c in coins if s - c in best]
        if cand:
            best[s] = min(cand, key=len)
    lanes = best.get(total)
    return lanes if lanes is not None and len(lanes) <= nlanes else None
