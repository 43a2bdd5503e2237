"""numpy restatement of clrrt_tree_rebase's bookkeeping (include/clrrt.h): subtree membership and the descendant
closure with revalidation, renumbering, costE' and the row heading / time subtractions.  No test functions here.

What it does not restate is pinned by the engine's own entries (tests/test_rebase_gpu.py): header and row (x, y) bits
by path_load + path_transform + path_download, row validity by clrrt_obstacle_distance, costS' and goal by
clrrt_tree_init_from_path on loaded chains.

The closure is pointer doubling over `parent`, as the device runs it; tests/test_rebase_host.py checks it against the
naive loop (parents precede children, so one pass in id order decides every node).
"""
import numpy as np


def closure(parent, root, invalid=None):
    """(member, kept, level, passes): member[k] -- k is root or its parent chain reaches root; kept[k] -- member, and
    no node on the chain from k up to (not including) root is invalid (root itself is always kept here: the caller
    handles an invalid root); level[k] -- hops from k to root (members only, else -1); passes -- doubling passes run,
    the last of which moved nothing."""
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    bad = np.zeros(n, dtype=bool) if invalid is None else np.asarray(invalid, dtype=bool).copy()
    jump = parent.copy()
    jump[root] = -1
    hop = np.where((jump < 0), 0, 1).astype(np.int64)
    passes = 0
    while True:
        passes += 1
        act = np.flatnonzero((jump >= 0) & (jump != root))
        if len(act) == 0:
            break
        j = jump[act]
        nb, nh, nj = bad[act] | bad[j], hop[act] + hop[j], jump[j]  # (read everything before writing: double buffer)
        bad[act], hop[act], jump[act] = nb, nh, nj
    member = jump == root
    member[root] = True
    kept = member & ~bad
    kept[root] = True
    level = np.where(member, hop, -1)
    level[root] = 0
    return member, kept, level, passes


def closure_naive(parent, root, invalid=None):
    """The same (member, kept, level) by one loop in id order."""
    n = len(parent)
    member, kept, level = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int64)
    member[root] = kept[root] = True
    level[root] = 0
    for k in range(root + 1, n):
        p = int(parent[k])
        if p >= 0 and member[p]:
            member[k] = True
            level[k] = level[p] + 1
            kept[k] = kept[p] and not (invalid is not None and invalid[k])
    return member, kept, level


def renumber(kept, parent, root):
    """(old ids of the kept nodes in order, new parent per kept node): the new id is the rank among the kept nodes."""
    ids = np.flatnonzero(kept)
    new_id = np.cumsum(kept) - 1
    par = np.where(ids == root, -1, new_id[np.asarray(parent)[ids]]).astype(np.int32)
    return ids, par


def cost_e(costE, root):
    """costE' = (float)((double)costE - (double)costE[root])."""
    c = np.asarray(costE, dtype=np.float32)
    return (c.astype(np.float64) - np.float64(c[root])).astype(np.float32)


def shift_rows(rows_xy_done, pose, t_shift):
    """Rows whose (x, y) are already in the new frame: heading - pose[2], time - t_shift."""
    r = np.array(rows_xy_done, dtype=np.float64, copy=True)
    r[:, 2] = r[:, 2] - np.float64(pose[2])
    r[:, 6] = r[:, 6] - np.float64(t_shift)
    return r


def node_rows(nodes, ids, root):
    """(first row, row count) in the old arena of each kept node: the root keeps only its last row."""
    off = np.asarray(nodes["row_offset"], dtype=np.int64)[ids].copy()
    nr = np.asarray(nodes["nrows"], dtype=np.int64)[ids].copy()
    r = np.flatnonzero(ids == root)
    off[r] += nr[r] - 1
    nr[r] = 1
    return off, nr
