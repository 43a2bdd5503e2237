"""Can the rollout queue be ordered by predicted chain length, and what would that buy?  (Step 0 of the
length-class queue order)

Grow a cfg3 tree for argv[1] rounds (default 40), draw one round of 16384 samples, take their candidate lists and
simulate every candidate; every successful regular rollout that passes the goal-bias gate is followed by its
goal-biased rollout, as in k_roll_run.  That gives each job's chain length in steps.  The tool then
  1. tabulates chain length against what is known before the rollout runs (distance from the parent to the sample,
     the parent's speed, the bearing of the sample off the parent's heading, the goal-bias gate evaluated at the
     sample),
  2. fits and scores a closed-form predictor of the expected chain length (L) and the class rule the tables lead to
     (Q, the one k_roll_flag implements),
  3. replays the actual lengths through a host model of the persistent queue (W waves x 64 lanes, refill at
     REFILL_MIN parked or idle lanes, cap T, fetch skipped and rollouts abandoned after an earlier candidate's
     success) under the present order, the predicted-class order and perfect longest-first, and reports tail and
     total wave-steps per wave.
argv[2]: waves of the grid (default 384 = 96 blocks, the late-query width); argv[3]: output file (default stdout only);
`--save FILE.npz` keeps the jobs' arrays, `--load FILE.npz` repeats the analysis from them without a GPU.
`--selftest` runs the queue model on synthetic lengths without a GPU."""
import os
import sys

import numpy as np

T = 128          # defer_steps
REFILL_MIN = 16
ABANDON_EVERY = 16
K = 10           # CAND_K
NB = 8
# class c >= 1 holds predicted chain steps in [BOUNDS[c - 1], BOUNDS[c]); class 0 is "no candidate"; the top class is
# ">= T or orbit"
BOUNDS = [0, 23, 32, 45, 64, 91, 128]  # T / 2^(k/2)


def classes_of(pred, bounds=BOUNDS):
    return 1 + np.searchsorted(np.asarray(bounds[1:], dtype=np.float64), pred, side="right")


def simulate_queue(order, s_of, k_of, valid, reg_len, reg_ok, gb_len, W, carry=None, per_job=None):
    """One launch of the persistent queue.  order: job indices in queue order; job i is candidate k_of[i] of sample
    s_of[i], valid[i] 0 = no candidate (skipped at fetch); reg_len / reg_ok the regular rollout's steps and success,
    gb_len the goal-biased follow-up's steps (0: none).  carry: remaining steps of chains resumed at the queue's
    front; per_job (nullable): receives each job's lane-steps.  Returns (queue-phase wave-steps, tail wave-steps,
    lane-steps, tail lane-steps, makespan in steps)."""
    carry = np.zeros(0, dtype=np.int64) if carry is None else np.asarray(carry, dtype=np.int64)
    nc = len(carry)
    nq = nc + len(order)
    best = np.full(int(s_of.max()) + 1 if len(s_of) else 1, 1 << 30, dtype=np.int64)
    job = np.full((W, 64), -1, dtype=np.int64)    # -1 idle, -2 a carried chain, else job index
    rem = np.zeros((W, 64), dtype=np.int64)       # steps left in the current rollout
    steps = np.zeros((W, 64), dtype=np.int64)
    chain = np.zeros((W, 64), dtype=np.int64)
    ps = np.zeros((W, 64), dtype=np.int64)        # 0 regular, 1 goal-biased
    parked = np.zeros((W, 64), dtype=bool)
    qdone = np.zeros(W, dtype=bool)
    alive = np.ones(W, dtype=bool)
    qnext = 0
    ws = [0, 0]
    ls = [0, 0]
    t = 0
    while alive.any():
        busy = (job != -1) & ~parked
        idle = (job == -1) & ~qdone[:, None]
        npk = parked.sum(1)
        nbusy = busy.sum(1)
        trig = alive & ((npk + idle.sum(1)) > 0) & (((npk + idle.sum(1)) >= REFILL_MIN) | (nbusy == 0) | (qdone & (npk > 0)))
        for w in np.nonzero(trig)[0]:
            while True:
                # finish the parked lanes: record a success, start the follow-up or free the lane
                for l in np.nonzero(parked[w])[0]:
                    i = job[w, l]
                    parked[w, l] = False
                    if i >= 0 and ps[w, l] == 0 and rem[w, l] <= 0 and reg_ok[i]:
                        best[s_of[i]] = min(best[s_of[i]], k_of[i])
                        if gb_len[i] > 0:
                            ps[w, l] = 1
                            rem[w, l] = gb_len[i]
                            steps[w, l] = 0
                            continue
                    job[w, l] = -1
                il = np.nonzero((job[w] == -1))[0] if not qdone[w] else np.zeros(0, dtype=np.int64)
                if len(il) == 0:
                    break
                q0 = qnext + np.arange(len(il))
                qnext += len(il)
                if (q0 >= nq).any():
                    qdone[w] = True
                for l, q in zip(il, q0):
                    if q >= nq:
                        continue
                    if q < nc:
                        job[w, l] = -2
                        rem[w, l] = carry[q]
                    else:
                        i = order[q - nc]
                        if not valid[i] or best[s_of[i]] < k_of[i]:
                            continue
                        job[w, l] = i
                        rem[w, l] = reg_len[i]
                    steps[w, l] = 0
                    chain[w, l] = 0
                    ps[w, l] = 0
                nidle = int((job[w] == -1).sum())
                if qdone[w] or nidle < REFILL_MIN and (job[w] != -1).any():
                    break
        alive = ~(qdone & (job == -1).all(1))
        act = (job != -1) & ~parked & alive[:, None]
        # a chain at its cap is suspended instead of stepping
        cap = act & (chain >= T)
        parked |= cap
        act &= ~cap
        na = act.sum(1)
        stepping = na > 0
        for ph in (0, 1):
            m = stepping & (qdone == bool(ph))
            ws[ph] += int(m.sum())
            ls[ph] += int(na[m].sum())
        if not stepping.any():
            continue
        t += 1
        if per_job is not None:
            np.add.at(per_job, job[act & (job >= 0)], 1)
        steps[act] += 1
        chain[act] += 1
        rem[act] -= 1
        done = act & (rem <= 0)
        parked |= done
        # abandon check every ABANDON_EVERY steps
        chk = act & ~done & (job >= 0) & (steps % ABANDON_EVERY == 0)
        if chk.any():
            wi, li = np.nonzero(chk)
            ji = job[wi, li]
            drop = best[s_of[ji]] < k_of[ji]
            job[wi[drop], li[drop]] = -1
    return ws[0], ws[1], ls[0] + ls[1], ls[1], t


def report_orders(out, label, W, s_of, k_of, valid, reg_len, reg_ok, gb_len, chain_len, preds, q_cls, orbit):
    """The queue model under the present order, the orders of the predictors `preds` (name -> predicted steps,
    geometric classes), of the class arrays q_cls (name -> classes, nullable) and perfect longest-first."""
    B = int(s_of.max()) + 1
    q = k_of * B + s_of                       # present queue position (k-major)
    over = chain_len[valid & (chain_len > T)]  # chains a launch suspends: resumed at the front of the next one
    carry = np.minimum(over - T, T)
    n = len(s_of)
    orders = {}
    orders["present (orbit class first, else k-major)"] = np.lexsort((q, -(valid & orbit).astype(np.int64)))
    orders["plain (k-major)"] = np.argsort(q, kind="stable")
    for name, pred in preds.items():
        orders[f"{name}, {NB} geometric classes"] = np.lexsort((q, -np.where(valid, classes_of(pred), 0)))
        fine = np.where(valid, np.minimum(pred, T).astype(np.int64) // 8 + 1, 0)
        orders[f"{name}, 17 bins of 8 steps"] = np.lexsort((q, -fine))
    for name, cls in (q_cls or {}).items():
        orders[name] = np.lexsort((q, -np.where(valid, cls, 0)))
    orders["perfect longest-first (actual lengths)"] = np.lexsort((q, -np.where(valid, np.minimum(chain_len, T), -1)))
    base = None
    for name, o in orders.items():
        assert len(o) == n
        wq, wt, lanes, lanes_t, mk = simulate_queue(o, s_of, k_of, valid, reg_len, reg_ok, gb_len, W, carry)
        tot = wq + wt
        base = base or (tot, lanes)
        out(f"  {label} {name}: per wave {wq / W:.1f} queue-phase + {wt / W:.1f} tail = {tot / W:.1f} wave-steps "
            f"({(tot / base[0] - 1) * 100:+.1f}%), makespan {mk} steps, lane-steps {lanes} (x{lanes / base[1]:.3f}; tail "
            f"{lanes_t}), utilisation {lanes / max(1, tot) / 64:.2f}")


def selftest():
    rng = np.random.default_rng(1)
    B = 4096
    s_of = np.repeat(np.arange(B), K)
    k_of = np.tile(np.arange(K), B)
    valid = rng.random(B * K) < 0.9
    reg_len = np.minimum(rng.exponential(34, B * K).astype(np.int64) + 1, 1000)
    reg_ok = rng.random(B * K) < 0.3
    gb_len = np.where(reg_ok & (rng.random(B * K) < 0.2), rng.integers(20, 300, B * K), 0)
    chain_len = reg_len + gb_len
    pred = chain_len * rng.uniform(0.6, 1.4, B * K)
    report_orders(print, "selftest", 96, s_of, k_of, valid, reg_len, reg_ok, gb_len, chain_len, {"noisy": pred}, None,
                  rng.random(B * K) < 0.03)


def gate_at(P, x, y, bx, by):
    """feasible_goal_bias (rrtplanner.cpp:292-) for a vehicle at (x, y) whose reference ends at (bx, by)."""
    g = P.goal
    R1 = 4.77
    lx = g[0] + R1 * np.cos(g[2] - np.pi / 2)
    rx = g[0] + R1 * np.cos(g[2] + np.pi / 2)
    ly, ry = g[1] + R1 * np.cos(g[2] - np.pi / 2), g[1] + R1 * np.cos(g[2] + np.pi / 2)
    outl = np.hypot(x - lx, y - ly) > R1 - 0.3
    outr = np.hypot(x - rx, y - ry) > R1 - 0.3
    aref = np.arctan2(g[1] - by, g[0] - bx)
    wrap = lambda a: np.mod(a + np.pi, 2 * np.pi) - np.pi  # noqa: E731
    m = np.minimum(np.abs(wrap(g[2] - aref)), np.abs(wrap(g[2] + np.pi - aref)))
    return outl & outr & (m < np.pi / 8)


def main():
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
    import clrrt
    from clrrt import abi, scenes

    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 384
    fout = open(sys.argv[3], "a") if len(sys.argv) > 3 else None

    def out(s):
        print(s, flush=True)
        if fout:
            fout.write(s + "\n")
            fout.flush()

    B = 16384
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=6 << 20,
                       max_rows=(6 << 20) * 48, max_batch=B)
    pl.set_obstacles(scenes.urban_scene(200))
    pl.set_option("defer_steps", T)
    pl.tree_init()
    pl.expand(clrrt.Rng(5), n_iters=rounds * B, budget_ms=1e9, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
    nd = pl.nodes()
    P = pl.params
    smp = list(clrrt.Rng(77).draw_samples(P, B))
    ids, _ = pl.sort_nodes_batch(smp, exact=False)
    sxy = np.array([(s.x, s.y) for s in smp])
    s_of = np.repeat(np.arange(B), K)
    k_of = np.tile(np.arange(K), B)
    par = ids.reshape(-1).astype(np.int64)
    valid = par >= 0
    vi = np.nonzero(valid)[0]
    jobs = [(int(par[i]), 0, float(sxy[s_of[i], 0]), float(sxy[s_of[i], 1])) for i in vi]
    res = pl.simulate_batch(jobs)
    n = B * K
    reg_len = np.zeros(n, dtype=np.int64)
    reg_ok = np.zeros(n, dtype=bool)
    gb_len = np.zeros(n, dtype=np.int64)
    outc = np.full(n, -1, dtype=np.int64)
    reg_len[vi] = [r["nrows"] - 1 for r in res]
    outc[vi] = [r["outcome"] for r in res]
    reg_ok[vi] = (outc[vi] == 1) | (outc[vi] == 2)
    fin = np.zeros((n, 10)); rb = np.zeros((n, 2)); rvb = np.zeros(n)
    fin[vi] = [r["final"] for r in res]
    rb[vi] = [r["ref_back"] for r in res]
    rvb[vi] = [r["ref_vback"] for r in res]
    follow = np.nonzero(reg_ok & gate_at(P, fin[:, 0], fin[:, 1], rb[:, 0], rb[:, 1]))[0]
    for c0 in range(0, len(follow), 2048):
        ch = follow[c0:c0 + 2048]
        r2 = pl.simulate([(fin[i], rb[i, 0], rb[i, 1], 0.0, 0.0, 0, 1, rvb[i]) for i in ch], ref_cap=8)
        gb_len[ch] = [max(1, r["nrows"] - 1) for r in r2]
    chain_len = reg_len + gb_len

    out(f"== cfg3 after {rounds} rounds: tree {pl.size()[0]} nodes, {int(valid.sum())} candidates of {B} samples, "
        f"{len(follow)} goal-biased follow-ups; W = {W} waves, T = {T}")
    cl = chain_len[valid]
    out(f"chain steps: mean {cl.mean():.1f}, p50 {np.percentile(cl, 50):.0f}, p90 {np.percentile(cl, 90):.0f}, p99 "
        f"{np.percentile(cl, 99):.0f}; >= 60: {(cl >= 60).mean() * 100:.1f}%, >= {T}: {(cl >= T).mean() * 100:.1f}%; regular "
        f"mean {reg_len[valid].mean():.1f}; follow-ups mean {gb_len[follow].mean() if len(follow) else 0:.1f}; outcomes "
        f"{np.bincount(outc[valid], minlength=5).tolist()}")

    # features known before the rollout
    st = nd["state"][np.maximum(par, 0)]
    pbx, pby = nd["ref_back"][np.maximum(par, 0), 0], nd["ref_back"][np.maximum(par, 0), 1]
    sx, sy = sxy[s_of, 0], sxy[s_of, 1]
    dpos = np.hypot(sx - st[:, 0], sy - st[:, 1])
    dref = np.hypot(sx - pbx, sy - pby)
    v0 = st[:, 4]
    ang = np.abs(np.mod(np.arctan2(sy - st[:, 1], sx - st[:, 0]) - st[:, 2] + np.pi, 2 * np.pi) - np.pi)
    gate_s = gate_at(P, sx, sy, sx, sy)
    dgoal = np.hypot(P.goal[0] - sx, P.goal[1] - sy)
    orbit = (dpos >= 8) & (dpos < 20) & (ang >= np.pi / 6) & (ang < np.pi / 2)
    cc = np.minimum(chain_len, T).astype(np.float64)

    def table(name, x, edges):
        out(f"chain steps (capped at {T}) by {name}: bin, jobs, mean, p50, p90, share >= 60")
        for a, b in zip(edges[:-1], edges[1:]):
            m = valid & (x >= a) & (x < b)
            if m.sum() == 0:
                continue
            out(f"  {a:7.2f}-{b:7.2f} {int(m.sum()):7d} {cc[m].mean():6.1f} {np.percentile(cc[m], 50):5.0f} "
                f"{np.percentile(cc[m], 90):5.0f} {(cc[m] >= 60).mean() * 100:5.1f}%")

    table("|sample - parent ref.back()| (m)", dref, [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 1e9])
    table("|sample - parent position| (m)", dpos, [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 1e9])
    table("parent speed (m/s)", v0, [0, 0.5, 1, 2, 3, 4, 5, 1e9])
    table("bearing off heading (deg)", np.degrees(ang), [0, 15, 30, 60, 90, 120, 150, 181])
    table("goal-bias gate at the sample (0 / 1)", gate_s.astype(float), [0, 0.5, 1.5])
    table("orbit class of roll_orbit_class (0 / 1)", orbit.astype(float), [0, 0.5, 1.5])
    m = valid & gate_s
    out(f"gate at the sample: {int(m.sum())} jobs; of the follow-ups run, {gate_s[follow].mean() * 100 if len(follow) else 0:.1f}% "
        f"had it set; jobs with it set that ran a follow-up: {(gb_len[m] > 0).mean() * 100 if m.sum() else 0:.1f}%")
    table("distance sample - goal (m), gate set", np.where(gate_s, dgoal, -1.0), [0, 5, 10, 15, 20, 30, 40, 1e9])

    analyse(out, rounds, W, s_of, k_of, valid, reg_len, reg_ok, gb_len, outc, dpos, dref, v0, ang, gate_s, dgoal, orbit)
    if "--save" in sys.argv:
        np.savez_compressed(sys.argv[sys.argv.index("--save") + 1], rounds=rounds, W=W, s_of=s_of, k_of=k_of, valid=valid,
                            reg_len=reg_len, reg_ok=reg_ok, gb_len=gb_len, outc=outc, dpos=dpos, dref=dref, v0=v0, ang=ang,
                            gate_s=gate_s, dgoal=dgoal, orbit=orbit)


def lsq(terms, y, m):
    X = np.stack(terms, 1)
    coef, *_ = np.linalg.lstsq(X[m], y[m], rcond=None)
    return coef, X @ coef


def analyse(out, rounds, W, s_of, k_of, valid, reg_len, reg_ok, gb_len, outc, dpos, dref, v0, ang, gate_s, dgoal, orbit):
    """Predictors of the chain length and the queue model under the orders they give."""
    n = len(s_of)
    chain_len = reg_len + gb_len
    cc = np.minimum(chain_len, T).astype(np.float64)
    one = np.ones(n)
    vv = np.maximum(v0, 0.5)
    preds = {}

    def score(name, p, text):
        r = np.corrcoef(p[valid], cc[valid])[0, 1]
        longm = valid & (cc >= 60)
        out(f"predictor {name}: {text}; corr {r:.3f}; chains >= 60 predicted >= 45: {(p[longm] >= 45).mean() * 100:.1f}%, "
            f"chains < 23 predicted >= 45: {(p[valid & (cc < 23)] >= 45).mean() * 100:.1f}%")
        cls = classes_of(p)
        out("  class (predicted): jobs, mean actual, p90 actual, max actual: " + "; ".join(
            f"{c}: {int((valid & (cls == c)).sum())}, {cc[valid & (cls == c)].mean():.0f}, "
            f"{np.percentile(cc[valid & (cls == c)], 90):.0f}, {cc[valid & (cls == c)].max():.0f}"
            for c in range(1, NB) if (valid & (cls == c)).sum()))
        preds[name] = p

    # L: the expected chain length, one least-squares fit over every job
    tl = ["1", "dpos", "dpos/v", "ang", "gate", "gate*dgoal"]
    coef, p = lsq([one, dpos, dpos / vv, ang, gate_s.astype(float), gate_s * dgoal], cc, valid & ~orbit)
    p = np.clip(p, 0, T - 1)
    p[orbit] = T
    score("L (expected length, linear)", p, "coefficients " + ", ".join(f"{t} {c:+.3f}" for t, c in zip(tl, coef)))
    miss = valid & (cc >= 60) & (p < 45)
    if miss.sum():
        out(f"  missed by L (actual >= 60, predicted < 45): {int(miss.sum())} jobs; follow-up ran {100 * (gb_len[miss] > 0).mean():.0f}%, "
            f"gate at sample {100 * gate_s[miss].mean():.0f}%, iteration limit {100 * (outc[miss] == 0).mean():.0f}%, "
            f"dpos p50 {np.median(dpos[miss]):.1f} m, v0 p50 {np.median(v0[miss]):.2f}, bearing p50 "
            f"{np.degrees(np.median(ang[miss])):.0f} deg")

    # Q: what the tables say.  The jobs fall into two populations.  A parent at rest (v < 0.5: the root and its
    # zero-length children) makes a "steady" chain: ~60 steps of acceleration before anything can end it, 75 steps
    # typical, little spread -- except toward a sample closer than 7 m or >= 45 degrees off the heading, or (less
    # often) nearly straight ahead, where the chain often reaches the cap.  A moving parent makes a "heavy-tailed"
    # chain: a step or two (an early collision, or the sample reached) in nine cases of ten, but 2-3% run >= 60
    # steps (a late collision, a long goal-biased follow-up) and nothing known beforehand tells which.  All ten
    # candidates of a sample are alike, so a class that holds them all runs them side by side and the later ones
    # no longer find the earlier one's success at fetch: the classes are formed per half of the candidate list.
    # Classes (k_roll_flag): 7 first half heavy-tailed, orbits, candidate 0 of a standing start likely to reach the
    # cap; 6 / 5 first half steady (straight ahead / the rest); 4 the other candidates of cap-likely standing starts;
    # 3 second half heavy-tailed; 2 / 1 second half steady.  Q1 is the same without the halves.
    slow = v0 < 0.5
    deg = np.degrees(ang)
    out("standing starts (parent speed < 0.5): chains of >= 100 steps by |sample - parent position| (m) and by bearing "
        "(deg): bin, jobs, share >= 100, p50, p90")
    for nm, x, edges in (("distance", dpos, [0, 2, 4, 7, 10, 12, 16, 24, 40, 1e9]),
                         ("bearing", deg, [0, 5, 10, 15, 20, 30, 45, 60, 90, 181])):
        for a, b in zip(edges[:-1], edges[1:]):
            mm = valid & slow & (x >= a) & (x < b)
            if mm.sum():
                out(f"  {nm} {a:5.0f}-{b:5.0f} {int(mm.sum()):7d} {(cc[mm] >= 100).mean() * 100:5.1f}% "
                    f"{np.percentile(cc[mm], 50):5.0f} {np.percentile(cc[mm], 90):5.0f}")
    mv = valid & ~slow
    out(f"moving parents: {int(mv.sum())} jobs, chain mean {cc[mv].mean():.1f}, p50 {np.percentile(cc[mv], 50):.0f}, p90 "
        f"{np.percentile(cc[mv], 90):.0f}, >= 60: {(cc[mv] >= 60).mean() * 100:.1f}% ({int((mv & (cc >= 60)).sum())} jobs; by the "
        f"follow-up {int((mv & (cc >= 60) & (reg_len < 60)).sum())}); with the gate at the sample "
        f"{(cc[mv & gate_s] >= 60).mean() * 100:.1f}%, without {(cc[mv & ~gate_s] >= 60).mean() * 100:.1f}%")
    hi = slow & ((dpos < 7) | (deg >= 45))
    mid = slow & ~hi & (deg < 10)
    lo = slow & ~hi & ~mid
    half0 = k_of < K // 2
    q1_cls = np.where(hi | (~slow & orbit), 7, np.where(~slow, 4, np.where(mid, 3, 2)))
    q_cls = np.where(~slow, np.where(half0 | orbit, 7, 3),
                     np.where(hi, np.where(k_of == 0, 7, 4), np.where(mid, np.where(half0, 6, 2), np.where(half0, 5, 1))))
    for nm, mm in (("standing start, near or wide (likely to reach the cap)", hi), ("standing start, straight ahead", mid),
                   ("standing start, the rest", lo), ("moving parent", ~slow)):
        mm = valid & mm
        if mm.sum():
            out(f"  {nm}: {int(mm.sum())} jobs, rollouts succeeding {reg_ok[mm].mean() * 100:.0f}%, actual chain mean {cc[mm].mean():.0f}, "
                f"p50 {np.percentile(cc[mm], 50):.0f}, p90 {np.percentile(cc[mm], 90):.0f}, p99 {np.percentile(cc[mm], 99):.0f}, "
                f">= 100: {(cc[mm] >= 100).mean() * 100:.1f}%")
    okm = (reg_ok & valid).reshape(-1, K)
    first = np.where(okm.any(1), okm.argmax(1), K - 1)
    need = valid & (k_of <= first[s_of])
    out(f"  lane-steps if every candidate ran: {int(cc[valid].sum())}; of the candidates up to each sample's first success "
        f"alone: {int(cc[need].sum())}")
    out("queue model")
    report_orders(out, f"[{rounds} rounds]", W, s_of, k_of, valid, reg_len, reg_ok, gb_len, chain_len, preds, {"Q1 (cap-likely, heavy-tailed, steady)": q1_cls,
                   "Q (the same per half of the candidate list)": q_cls}, orbit)


if __name__ == "__main__":
    if "--selftest" in sys.argv:
        selftest()
    elif "--load" in sys.argv:  # the analysis alone, from arrays a GPU run saved with --save
        z = dict(np.load(sys.argv[sys.argv.index("--load") + 1]))
        analyse(print, int(z.pop("rounds")), int(z.pop("W")), **z)
    else:
        main()
