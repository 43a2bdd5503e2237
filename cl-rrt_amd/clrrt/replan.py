"""Config 5 replanning loop (BASELINE.json configs[4]; SURVEY.md §8(d) "Cfg 5"): 5 Hz planMotion
queries with the tree re-initialised from the previous best path (commit_path = 1).

One query follows MotionPlanner::planMotion (rrt/src/motionplanner.cpp:8-77):
    carPose = transformStateToLocal(worldState)                      :14-15  (x, y, heading -> 0)
    transformNodesWorldToCar(bestNodes, worldState)                   :22
    initializeTree(RRT, veh, bestNodes, carPose)                      :32
    for (Timer timer(200); timer.Get(); ) expandTree(...)             :39-43
    bestNodes = extractBestPath(RRT.tree)                             :51
    transformNodesCarToworld(bestNodes, worldState)                   :54
The scenario around it is this benchmark's, not the reference's (the reference takes its state,
goal and obstacles from ROS topics): a fixed world goal and obstacle set, moving obstacles advanced
at their velocity, both handed to each query in the car frame, and the ego moved 0.2 s along the
committed path between queries.  Backends: the HIP planner (`PlannerBackend`) and, in the tests,
the CPU oracle through the same five calls.
"""
import math

import numpy as np

from . import abi

QUERY_PERIOD = 0.2  # 5 Hz


def world_to_car_pose(x, y, pose):
    """transformPointWorldToCar (transformations.cpp:6-11), vectorised."""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return (x * c - pose[0] * c - pose[1] * s + y * s, y * c - pose[1] * c + pose[0] * s - x * s)


def obstacles_in_car_frame(obs_world, t, pose):
    """World obstacles (cx, cy, theta, size_x, size_y, vx, vy) at time t, in the car frame of `pose`
    (centre transformed, heading and velocity rotated -- rotateVelocityVector, transformations.cpp:318)."""
    o = np.array(obs_world, dtype=np.float64).reshape(-1, 7)
    cx, cy = o[:, 0] + o[:, 5] * t, o[:, 1] + o[:, 6] * t
    o[:, 0], o[:, 1] = world_to_car_pose(cx, cy, pose)
    o[:, 2] = o[:, 2] - pose[2]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    vx, vy = o[:, 5].copy(), o[:, 6].copy()
    o[:, 5], o[:, 6] = c * vx + s * vy, -s * vx + c * vy
    return o


def goal_in_car_frame(goal_world, pose):
    gx, gy = world_to_car_pose(np.array([goal_world[0]]), np.array([goal_world[1]]), pose)
    return (float(gx[0]), float(gy[0]), float(goal_world[2] - pose[2]), float(goal_world[3]))


def advance_pose(pose, path_rows, dt=QUERY_PERIOD):
    """The ego after `dt` s along the committed path (rows in world x, y; row headings stay in the
    car frame of the query that grew them, as transformNodesCarToworld leaves them).  No path: keep
    going straight at the current speed."""
    if path_rows is None or len(path_rows) == 0:
        v = pose[4]
        return np.array([pose[0] + v * dt * math.cos(pose[2]), pose[1] + v * dt * math.sin(pose[2]), pose[2],
                         pose[3], v, pose[5]])
    t0 = path_rows[0, 6]
    k = int(np.searchsorted(path_rows[:, 6] - t0, dt - 1e-9))
    k = min(k, len(path_rows) - 1)
    r = path_rows[k]
    return np.array([r[0], r[1], pose[2] + r[2], r[3], r[4], r[5]])


class PlannerBackend:
    """The five planMotion steps on the HIP planner (clrrt.Planner).  complete_path: with a sharded planner, the
    collective that completes the committed path's rows across the ranks, called in every query between path_commit
    and path_transform with the planner (clrrt.dist.NativeExchange.path_rows, or
    lambda pl: clrrt.dist.fetch_path_rows(pl, rank)); its result (rows moved) is kept in rows_fetched.

    carry_tree (engine extension, default False: nothing changes): the tree is kept between queries instead of being
    cut down to the committed path.  begin_query then picks as new root the tree id of the first committed-path node
    that initializeTree's filter would keep (its last row has x >= 0 in the new car frame), calls
    Planner.tree_rebase with the new car pose expressed in the previous car frame and t_shift = that node's state[6],
    and falls back to tree_init_from_path when there is no such node or the root's row collides.  The committed path is
    transformed either way.  last_rebase: the rebase info of the last query that carried its tree (else None).  Not
    with a sharded planner."""

    def __init__(self, planner, make_params, complete_path=None, carry_tree=False):
        if carry_tree and complete_path is not None:
            raise ValueError("carry_tree is not supported with a sharded planner")
        self.pl = planner
        self.make_params = make_params
        self.complete_path = complete_path
        self.rows_fetched = 0
        self.carry_tree = carry_tree
        self.last_rebase = None
        self._carry = None  # (previous pose, path ids, last world row per path node, state[6] per path node)

    def _carry_root(self, pose):
        """(tree id, t_shift) of the first committed-path node whose last row has x >= 0 in the car frame of `pose`
        (the nodes initializeTree keeps, rrtplanner.cpp:51-57: NaN is kept), or None."""
        _, ids, last_rows, times = self._carry
        for i, tree_id in enumerate(ids):
            x, _ = world_to_car_pose(last_rows[i, 0], last_rows[i, 1], pose)
            if not x < 0:
                return tree_id, times[i]
        return None

    def begin_query(self, pose, goal_car, obs_car):
        self.pl.set_params(self.make_params(pose[4], goal_car))
        self.pl.set_obstacles(obs_car)
        self.pl.path_transform(False, pose)
        self.last_rebase = None
        if self.carry_tree and self._carry is not None:
            root = self._carry_root(pose)
            if root is not None:
                prev = self._carry[0]
                px, py = world_to_car_pose(pose[0], pose[1], prev)
                info = self.pl.tree_rebase(root[0], [px, py, pose[2] - prev[2]], root[1])
                if info["outcome"] == abi.REBASE_KEPT:
                    self.last_rebase = info
                    return abi.REINIT_KEPT
        return self.pl.tree_init_from_path([0.0, 0.0, 0.0, pose[3], pose[4], pose[5]])

    def end_query(self, pose):
        ids, _, _ = self.pl.extract_best_path()
        self.pl.path_commit(ids)
        if self.complete_path is not None:
            self.rows_fetched = self.complete_path(self.pl)
        self.pl.path_transform(True, pose)
        nodes, rows = self.pl.path_download()
        if self.carry_tree:
            last = np.array([rows[nd.row_offset + nd.nrows - 1] for nd in nodes]).reshape(-1, 10)
            self._carry = (np.array(pose, dtype=np.float64), list(ids), last, [nd.state[6] for nd in nodes])
        return ids, rows


def run_queries(backend, expand, n_queries, obs_world, goal_world=(40.0, 0.0, 0.0, 0.0), v0=0.0,
                on_query=None):
    """Run n_queries replanning queries; `expand(q)` grows the tree of query q.  Returns the list of
    per-query (pose, outcome, path ids)."""
    pose = np.array([0.0, 0.0, 0.0, 0.0, v0, 0.0])
    log = []
    for q in range(n_queries):
        t = q * QUERY_PERIOD
        oc = backend.begin_query(pose, goal_in_car_frame(goal_world, pose), obstacles_in_car_frame(obs_world, t, pose))
        expand(q)
        ids, rows = backend.end_query(pose)
        log.append((pose.copy(), oc, list(ids)))
        if on_query is not None:
            on_query(q, pose, oc, ids)
        pose = advance_pose(pose, rows)
    return log


def default_make_params(collision_mode, vmax=5.0):
    def make(v0, goal_car):
        return abi.default_params(v0=v0, goal=goal_car, vmax=vmax, collision_mode=collision_mode)
    return make
