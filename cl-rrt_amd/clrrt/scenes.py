"""Synthetic urban scenes for the benchmark configs (SURVEY.md §8(d) scene generator).

uint32 LCG  s <- s*1664525 + 1013904223 (seed 12345); U(a, b) = a + (b - a) * (s >> 8) / 2**24.
Static obstacle: x = U(8, 60), y = U(-20, 20) (|y| < 3 -> y += 6), theta = U(-3.14, 3.14),
size_x = U(2, 6), size_y = U(4, 10), zero velocity.  Moving obstacles are drawn after the static
ones with the same fields (no lane shift) followed by vx = U(-2, 2), vy = U(-2, 2).
The LCG is independent of the planner's rand() stream.
"""
import numpy as np


class _Lcg:
    def __init__(self, seed=12345):
        self.s = seed & 0xFFFFFFFF

    def u(self, a, b):
        self.s = (self.s * 1664525 + 1013904223) & 0xFFFFFFFF
        return a + (b - a) * (self.s >> 8) / 16777216.0


def urban_scene(n_static, n_moving=0, seed=12345):
    """Returns an (M, 7) float64 array of obstacles: cx, cy, theta, size_x, size_y, vx, vy."""
    g = _Lcg(seed)
    out = []
    for _ in range(n_static):
        x = g.u(8.0, 60.0)
        y = g.u(-20.0, 20.0)
        if abs(y) < 3.0:
            y += 6.0
        th = g.u(-3.14, 3.14)
        sx = g.u(2.0, 6.0)
        sy = g.u(4.0, 10.0)
        out.append((x, y, th, sx, sy, 0.0, 0.0))
    for _ in range(n_moving):
        x = g.u(8.0, 60.0)
        y = g.u(-20.0, 20.0)
        th = g.u(-3.14, 3.14)
        sx = g.u(2.0, 6.0)
        sy = g.u(4.0, 10.0)
        vx = g.u(-2.0, 2.0)
        vy = g.u(-2.0, 2.0)
        out.append((x, y, th, sx, sy, vx, vy))
    return np.asarray(out, dtype=np.float64).reshape(-1, 7)


def rasterize(obstacles, x0, y0, res, w, h):
    """Occupancy cells (uint8 [h, w]) of the static obstacles' boxes: cell (i, j) is set when its centre
    (x0 + (i + 0.5) res, y0 + (j + 0.5) res) lies inside a box with zero velocity (the box of an obstacle:
    centre cx, cy, heading theta, size_y along the heading and size_x across it, each halved twice as
    getOBBvector does -- old_collisioncheck.cpp:6-22).  Moving obstacles are left out: they stay boxes."""
    obs = np.asarray(obstacles, dtype=np.float64).reshape(-1, 7)
    cx = x0 + (np.arange(w) + 0.5) * res
    cy = y0 + (np.arange(h) + 0.5) * res
    X, Y = np.meshgrid(cx, cy)
    out = np.zeros((h, w), dtype=bool)
    for ox, oy, th, sx, sy, vx, vy in obs:
        if vx != 0.0 or vy != 0.0:
            continue
        c, s = np.cos(th), np.sin(th)
        dx, dy = X - ox, Y - oy
        u = dx * c + dy * s
        v = dy * c - dx * s
        out |= (np.abs(u) <= sy / 4.0) & (np.abs(v) <= sx / 4.0)
    return out.astype(np.uint8)


def rasterize_layers(obstacles, x0, y0, res, w, h, layers, t0, dt, sub=4):
    """A stack of occupancy cells (uint8 [layers, h, w]) for set_occupancy_layers: layer k is rasterize's static cells
    plus every moving box at the times t = t0 + (k + s / sub) dt, s = 0 .. sub, of its slice -- centre + (vx, vy) t,
    heading fixed, as the OBB path predicts it -- rasterised the same way and united.  A scene generator for tests
    and tools, NOT a conservative sweep: a cell the box only crosses between two of the sampled times stays free."""
    obs = np.asarray(obstacles, dtype=np.float64).reshape(-1, 7)
    static = rasterize(obs, x0, y0, res, w, h).astype(bool)
    cx = x0 + (np.arange(w) + 0.5) * res
    cy = y0 + (np.arange(h) + 0.5) * res
    X, Y = np.meshgrid(cx, cy)
    out = np.zeros((layers, h, w), dtype=bool)
    for k in range(layers):
        out[k] = static
        for ox, oy, th, sx, sy, vx, vy in obs:
            if vx == 0.0 and vy == 0.0:
                continue
            c, sn = np.cos(th), np.sin(th)
            for s in range(sub + 1):
                t = t0 + (k + s / sub) * dt
                dx, dy = X - (ox + vx * t), Y - (oy + vy * t)
                u = dx * c + dy * sn
                v = dy * c - dx * sn
                out[k] |= (np.abs(u) <= sy / 4.0) & (np.abs(v) <= sx / 4.0)
    return out.astype(np.uint8)
