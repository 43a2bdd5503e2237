"""Query-space cases shared by tests/test_query_space_oracle.py (CPU) and tests/test_query_space.py (GPU).

Every other BATCH tree test runs one query (goal (40, 0, 0, 0), vmax 5, v0 0, sim_dt 0.04, root at rest), under
which no rollout comes near the horizon.  The cases here move the query: slow ones whose chains run to
2 n_steps_max and keep the deferral ring wrapping (LONG), and ones that move each parameter device code derives
something from -- feas_len, the sample region, n_steps_max, the bend / W2 / obs_use_pred branches, a moving
root (QUERY).  No test functions here: the tables, make(case), the oracle trees (grown once per (case, T) and
left unchanged) and the tree comparison.

Conventions: scene "M" = scenes.urban_scene(200, 20) with the OBB check, "S" = the stub check without
obstacles; the root is zeros with state[4] = v_root; the oracle is seeded with Oracle.srand(SEED), the device
with clrrt.Rng(SEED); oracle trees are grown with stable=True (the engine's BATCH order of equal keys).

The last entry of every case, "oracle", records what the oracle alone gave when the case was chosen (the
conditions test_query_space_oracle.py asserts are set well below these).
"""
import numpy as np

from clrrt import abi, scenes
from oracle_binding import Oracle

SEED = 7
COUNTERS = ("sim_count", "fail_collision", "fail_acclimit", "fail_iterlimit", "rollouts")

# ---- long chains (BATCH, B x rounds samples, defer_steps T): rounds > R = ceil(2 n_steps_max / T) + 2
LONG = {
    "slow_dt10_T16": dict(
        vmax=1.0, over=dict(sim_dt=0.1), scene="M", B=64, rounds=32, T=16,
        oracle="n_steps_max 200, R 27: 468 nodes, iterlimit 538, 15 accepted chains > 200, longest 379 (24 launches)"),
    "slow_dt10_T64": dict(
        vmax=1.0, over=dict(sim_dt=0.1), scene="M", B=128, rounds=14, T=64,
        oracle="n_steps_max 200, R 9: 524 nodes, iterlimit 505, 10 accepted chains > 200, longest 311 (5 launches)"),
    "slow_dt10_T16_stub": dict(
        vmax=1.5, over=dict(sim_dt=0.1), scene="S", B=64, rounds=32, T=16,
        oracle="n_steps_max 200, R 27: 2216 nodes, iterlimit 1860, 194 accepted chains > 200, longest 276 (18 launches)"),
    "slow_T128": dict(
        vmax=1.5, scene="M", B=128, rounds=14, T=128,
        oracle="n_steps_max 500, R 10: 686 nodes, 165 goal, iterlimit 206, 40 accepted chains > 500, longest 671 (6 launches)"),
    "slow_goal_T128_stub": dict(
        vmax=2.0, goal=(38.0, 3.0, 0.1, 0.5), scene="S", B=128, rounds=14, T=128,
        oracle="n_steps_max 500, R 10: 1992 nodes, 368 goal, iterlimit 1214, 87 accepted chains > 500, longest 860 (7 launches)"),
}

# ---- query space (BATCH, 256 x 4 rounds, each with T = 0 and T = 32)
QUERY_B, QUERY_ROUNDS, QUERY_TS = 256, 4, (0, 32)
_FAST = dict(v0=12.0, vmax=15.0, goal=(60.0, 0.0, 0.0, 8.0), v_root=12.0)   # ref_res 0.24: feas_len 0.504
QUERY = {
    "fast": dict(_FAST, scene="M", oracle="T 0 / T 32: 313 / 303 nodes, acclimit 912 / 1209"),
    "fast_stub": dict(_FAST, scene="S", oracle="1415 / 1051 nodes, 332 / 259 goal nodes"),
    # rollouts of at most 14 steps: shorter than T = 32, so nothing is deferred (the one case without deferrals)
    "fast_v20": dict(v0=20.0, vmax=25.0, goal=(90.0, 2.0, 0.0, 10.0), v_root=20.0, scene="M",   # ref_res 0.4
                     oracle="139 nodes, rollouts <= 14 steps (no deferral at T 32), acclimit 2288"),
    "goal_far": dict(v0=6.0, vmax=10.0, goal=(150.0, -20.0, -0.3, 3.0), v_root=6.0, scene="M",
                     oracle="122 nodes"),
    "goal_far_stub": dict(v0=6.0, vmax=10.0, goal=(150.0, -20.0, -0.3, 3.0), v_root=6.0, scene="S",
                          oracle="1733 / 1232 nodes, rows to 467"),
    "goal_near": dict(goal=(6.0, 1.0, 0.2, 0.0), v_root=2.0, scene="M", oracle="647 / 606 nodes, 92 / 64 goal nodes"),
    "goal_right": dict(goal=(30.0, -6.0, -0.4, 2.0), v_root=0.0, scene="M",
                       oracle="361 / 221 nodes, iterlimit 96 / 30"),
    "goal_left": dict(goal=(45.0, 8.0, 0.5, 1.0), v_root=1.0, scene="M", oracle="226 / 156 nodes"),
    "goal_36deg": dict(goal=(25.0, 18.0, 0.9, 0.0), v_root=2.0, scene="S", oracle="608 / 336 nodes"),
    "goal_m34deg": dict(goal=(30.0, -20.0, -0.7, 1.0), v_root=2.0, scene="S", oracle="632 / 331 nodes"),
    "dt02": dict(over=dict(sim_dt=0.02), v_root=0.0, scene="M", oracle="n_steps_max 1000: 271 / 170 nodes, rows to 286"),
    "dt10": dict(over=dict(sim_dt=0.1), v_root=0.0, scene="M", oracle="n_steps_max 200: 237 / 204 nodes"),
    "bend_w2": dict(over=dict(bend=1, lane_shift0=0.5, Cxy=(0.0, 0.05, -1.0), Wcost2=1.0), v_root=3.0, scene="M",
                    oracle="243 / 186 nodes"),
    "sort1": dict(over=dict(sort_limit=1), v_root=0.0, scene="M", oracle="200 / 170 nodes"),
    "nopred": dict(over=dict(obs_use_pred=0), v_root=0.0, scene="M", oracle="183 / 139 nodes"),
}
# the default query (test 4's first and third query)
DEFAULT = dict(scene="M")

NO_DEFERRAL = ("fast_v20",)


def case(name):
    if name == "default":
        return DEFAULT
    return LONG[name] if name in LONG else QUERY[name]


def _scene(kind):
    if kind == "S":
        return abi.CLRRT_COLLISION_STUB, None
    assert kind == "M", kind
    return abi.CLRRT_COLLISION_OBB, scenes.urban_scene(200, 20)


def make(c, scene=None):
    """case (a table entry or its name) -> (abi.Params, root_state[10], obstacles or None).  `scene` overrides
    the case's own ("M" / "S")."""
    if isinstance(c, str):
        c = case(c)
    mode, obs = _scene(scene or c["scene"])
    p = abi.default_params(v0=c.get("v0", 0.0), goal=c.get("goal", (40.0, 0.0, 0.0, 0.0)), vmax=c.get("vmax", 5.0),
                           collision_mode=mode)
    for k, v in c.get("over", {}).items():
        if k == "Cxy":
            for i in range(3):
                p.Cxy[i] = v[i]
        elif k == "Wcost2":
            p.Wcost[2] = v
        else:
            assert hasattr(p, k), k
            setattr(p, k, v)
    root = np.zeros(10)
    root[4] = c.get("v_root", 0.0)
    return p, root, obs


def n_steps_max(p):
    """The horizon of `for(i = 0; i < 20 / sim_dt; i++)` (simulation.cpp:58), as the engine's derive counts it."""
    n = 0
    while n < 20 / p.sim_dt:
        n += 1
    return n


def ring_slots(p, T):
    """Round slots of the deferral rings: a chain of at most 2 n_steps_max steps ends within ceil(2 n_steps_max / T)
    launches (+ 2)."""
    return -(-2 * n_steps_max(p) // T) + 2


def fresh_oracle(c, scene=None):
    """An oracle holding the case's root only, its rand() stream seeded."""
    p, root, obs = make(c, scene)
    o = Oracle(p, obs)
    Oracle.srand(SEED)
    o.init_tree(root)
    return o


_grown = {}


def grown(name, T=None, threads=16, B=None, rounds=None):
    """(oracle, samples deferred) of the case's BATCH expansion, grown once per key and left unchanged.  T: the
    case's own for a long-chain case, one of QUERY_TS otherwise."""
    c = case(name)
    if name in LONG:
        T = c["T"] if T is None else T
        B, rounds = B or c["B"], rounds or c["rounds"]
    else:
        B, rounds = B or QUERY_B, rounds or QUERY_ROUNDS
    key = (name, T, threads, B, rounds)
    if key not in _grown:
        o = fresh_oracle(c)
        ndef = o.expand_batch(B * rounds, B, stable=True, defer_steps=T, threads=threads)
        _grown[key] = (o, ndef)
    return _grown[key]


def accepted_chains(on):
    """Steps of every accepted chain, from the oracle's node table: nrows - 1 of a node, plus, for a goal-biased
    node (goal == 1 and parent == id - 1), nrows - 1 of its parent (the goal-biased rollout starts where the
    sample's own ended)."""
    nrows, par, goal = on["nrows"].astype(np.int64), on["parent"], on["goal"]
    ch = nrows - 1
    ids = np.arange(len(nrows))
    gb = (goal == 1) & (par == ids - 1) & (ids > 0)
    ch[gb] += nrows[par[gb]] - 1
    return ch[1:]


def first_divergence(on, gn):
    """Index of the first node whose header (parent, goal flag, row count, FP64 state bits) differs, or None."""
    n = min(len(on["parent"]), len(gn["parent"]))
    same = ((on["parent"][:n] == gn["parent"][:n]) & (on["goal"][:n] == gn["goal"][:n])
            & (on["nrows"][:n] == gn["nrows"][:n])
            & np.all(on["state"][:n].view(np.uint64) == gn["state"][:n].view(np.uint64), axis=1))
    bad = np.flatnonzero(~same)
    return int(bad[0]) if len(bad) else None


def assert_tree_equal(o, pl, label, rows=True):
    """The device tree of planner `pl` equals oracle `o`'s bit for bit: node headers, costE / costS bits, the five
    counters and (rows) every trajectory row."""
    on, gn = o.nodes(), pl.nodes()
    bad = first_divergence(on, gn)
    print(f"{label}: oracle {len(on['parent'])} nodes, gpu {len(gn['parent'])} nodes, first divergence {bad}")
    assert bad is None and len(on["parent"]) == len(gn["parent"]), (label, bad, len(on["parent"]), len(gn["parent"]))
    assert np.array_equal(gn["costE"].view(np.uint32), on["costE"].view(np.uint32)), label
    assert np.array_equal(gn["costS"].view(np.uint32), on["costS"].view(np.uint32)), label
    oc, gc = o.counters(), pl.counters()
    for k in COUNTERS:
        assert oc[k] == gc[k], (label, k, oc[k], gc[k])
    if rows:
        n_rows = pl.size()[1]
        all_rows = pl.rows(0, n_rows) if n_rows else np.zeros((0, 10))
        for i in range(1, len(on["parent"])):
            off, nr = int(gn["row_offset"][i]), int(gn["nrows"][i])
            got = all_rows[off:off + nr]
            assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(o.rows(i)).view(np.uint64)), (label, i)
    return on, gn
