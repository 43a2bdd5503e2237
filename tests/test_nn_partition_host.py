"""Tree-partitioned nearest-node search, host side (no GPU): the node ranges of clrrt.dist.node_range, the three
C-ABI entry points in the header and the binding, and the written definition of the list merge.

The merge (clrrt_nn_merge): per sample, the valid entries of every part list -- the first `count` of its 10 slots --
are ordered by (key, node id), keys compared as floats (`lex_less` in clrrt_kernels.hip; the keys are non-negative
finite Dubins distances or cost sums, so the order of their bit patterns is the same order), and the first
min(sort_limit, valid entries) of them are the result; slots past the count hold id -1 and key +inf.  Each part list
is itself the first sort_limit of its node range in that order, and the ranges are disjoint, so the first sort_limit
of the union is the first sort_limit of the whole tree: merging part lists of any partition gives the same list.
"""
import re
import subprocess

import numpy as np

import clrrt
from clrrt import dist as cdist

K = 10  # CAND_K: slots per list


def merge_model(ids, keys, counts, sort_limit):
    """ids / keys [parts][n][10], counts [parts][n] -> (ids [n][10], keys [n][10], counts [n])."""
    parts, n, _ = ids.shape
    out_i = np.full((n, K), -1, dtype=np.int32)
    out_k = np.full((n, K), np.inf, dtype=np.float32)
    out_n = np.zeros(n, dtype=np.int32)
    for s in range(n):
        ent = [(keys[p, s, j].view(np.uint32).item(), int(ids[p, s, j]))
               for p in range(parts) for j in range(int(counts[p, s]))]
        ent.sort()
        ent = ent[:sort_limit]
        out_n[s] = len(ent)
        for j, (kb, i) in enumerate(ent):
            out_i[s, j] = i
            out_k[s, j] = np.uint32(kb).view(np.float32)
    return out_i, out_k, out_n


def part_lists(keys_all, ranges, sort_limit):
    """The part lists a search of each node range returns: keys_all [n][N] (+inf = infeasible node)."""
    n = keys_all.shape[0]
    ids = np.full((len(ranges), n, K), -1, dtype=np.int32)
    keys = np.full((len(ranges), n, K), np.inf, dtype=np.float32)
    cnt = np.zeros((len(ranges), n), dtype=np.int32)
    for p, (first, count) in enumerate(ranges):
        for s in range(n):
            sub = keys_all[s, first:first + count]
            order = sorted((sub[i].view(np.uint32).item(), first + i) for i in range(count) if np.isfinite(sub[i]))
            order = order[:sort_limit]
            cnt[p, s] = len(order)
            for j, (kb, i) in enumerate(order):
                ids[p, s, j] = i
                keys[p, s, j] = np.uint32(kb).view(np.float32)
    return ids, keys, cnt


def test_node_range_tiles_the_tree():
    for n in (0, 1, 7, 4099):
        for world in (1, 2, 3, 8):
            nxt = 0
            for r in range(world):
                first, count = cdist.node_range(n, world, r)
                assert first == nxt and count >= 0, (n, world, r)
                assert (first, first + count) == (n * r // world, n * (r + 1) // world)
                nxt = first + count
            assert nxt == n
            # the same arithmetic as the sample slices
            assert [cdist.node_range(n, world, r) for r in range(world)] == [cdist.shard(n, world, r)
                                                                              for r in range(world)]


def test_partition_calls_declared_and_exported():
    names = ("clrrt_nn_range", "clrrt_nn_merge", "clrrt_round_eval_lists")
    txt = open(clrrt.HEADER_PATH).read()
    declared = set(re.findall(r"\b(clrrt_[a-z_0-9]+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", clrrt.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for s in names:
        assert s in declared, s
        assert s in exported, s
        assert s in clrrt.exported_symbols(), s
        assert hasattr(clrrt.lib(), s)
    assert re.search(r"#define\s+CLRRT_ABI_VERSION\s+11\b", txt)  # additive: the version stays
    for meth in ("nn_range", "nn_merge", "round_eval_lists"):
        assert callable(getattr(clrrt.Planner, meth))
    assert callable(cdist.PartitionedSearch)


def test_merge_model_agrees_across_partitions():
    rng = np.random.default_rng(3)
    n, N = 40, 137
    for sort_limit in (10, 4, 1):
        # keys drawn from a small set: plenty of equal keys, ordered by id; some nodes infeasible; samples 0-2 see
        # fewer feasible nodes than sort_limit
        keys_all = rng.integers(0, 12, size=(n, N)).astype(np.float32) * np.float32(0.37)
        keys_all[rng.random((n, N)) < 0.3] = np.inf
        keys_all[0, :] = np.inf
        keys_all[1, 3:] = np.inf
        keys_all[2, : N - 2] = np.inf
        whole = part_lists(keys_all, [(0, N)], sort_limit)
        want = merge_model(*whole, sort_limit)
        assert np.array_equal(want[0], whole[0][0]) and np.array_equal(want[2], whole[2][0])
        assert want[2][0] == 0 and want[2][1] <= min(3, sort_limit) and want[2][2] <= 2
        partitions = [[cdist.node_range(N, w, r) for r in range(w)] for w in (2, 3, 8)]
        partitions.append([(0, 1), (1, 4), (5, N - 5)])
        partitions.append([(0, 31), (31, 2), (33, 0), (33, N - 33)])  # an empty range
        for ranges in partitions:
            got = merge_model(*part_lists(keys_all, ranges, sort_limit), sort_limit)
            assert np.array_equal(got[0], want[0]), ranges
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), ranges
            assert np.array_equal(got[2], want[2]), ranges
            for s in range(n):  # strictly ascending (key bits, id); -1 / +inf past the count
                c = got[2][s]
                pairs = [(got[1][s, j].view(np.uint32).item(), got[0][s, j]) for j in range(c)]
                assert pairs == sorted(set(pairs))
                assert (got[0][s, c:] == -1).all() and np.isinf(got[1][s, c:]).all()
