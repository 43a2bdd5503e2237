"""Tree-partitioned nearest-node search (clrrt_nn_range, clrrt_nn_merge, clrrt_round_eval_lists, clrrt.dist
PartitionedSearch) -- GPU.

Every rank searches all samples of a round over its contiguous 1/W of the node ids, the per-range lists are merged in
(key, node id) order and the round's rollouts run from the merged lists.  The ranges are disjoint and each part list is
its range's first sort_limit entries in one total order, so the merged list is the list a search of the whole tree
returns (tests/test_nn_partition_host.py holds the written definition) and the rounds grow the same tree bit for bit.
"""
import ctypes as C
import datetime
import os
import re
import socket
import sys

import numpy as np
import pytest

import clrrt
from clrrt import abi, scenes
from clrrt import dist as cdist

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12
K = 10
NS = 777  # fresh samples: no multiple of 64, explore and optimize mixed

CONFIGS = {
    "walk": dict(nn_walk_min=64),  # ranges shorter than 64 nodes take the brute force inside the same partition
    "brute": dict(nn_walk_min=1 << 40),
    "overflow": dict(nn_walk_min=64, nn_walk_budget_tiles=1, nn_walk_budget_keys=1),  # every sample overflows
}


def _planner(opts, sort_limit=10, max_nodes=1 << 15, max_rows=1 << 25, max_batch=2048):
    p = clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB)
    p.sort_limit = sort_limit
    pl = clrrt.Planner(p, max_nodes=max_nodes, max_rows=max_rows, max_batch=max_batch)
    for k, v in opts.items():
        pl.set_option(k, v)
    pl.set_obstacles(scenes.urban_scene(200))
    pl.tree_init()
    return pl


def _grown(opts, sort_limit=10):
    """The tree of 5 BATCH rounds of 2048 samples (one more round while it has <= 2048 nodes)."""
    pl = _planner(opts, sort_limit)
    rng = clrrt.Rng(SEED)
    pl.expand(rng, n_iters=5 * 2048, mode=clrrt.CLRRT_MODE_BATCH, batch=2048)
    while pl.size()[0] <= 2048:
        pl.expand(rng, n_iters=2048, mode=clrrt.CLRRT_MODE_BATCH, batch=2048)
    return pl


def _fresh_samples(pl):
    smp = clrrt.Rng(77).draw_samples(pl.params, NS)
    ex = sum(s.explore for s in smp)
    assert 0 < ex < NS
    return smp


def _partitions(N):
    ps = {f"W{w}": [cdist.node_range(N, w, r) for r in range(w)] for w in (1, 2, 3, 8)}
    ps["root"] = [(0, 1), (1, 4), (5, N - 5)]  # the root alone, then fewer nodes than sort_limit
    ps["tiles"] = [(0, 31), (31, 2), (33, 1024), (1057, N - 1057)]  # a 32-node tile and a super-tile boundary
    ps["empty"] = [(0, N // 2), (N // 2, 0), (N // 2, N - N // 2)]
    return ps


_ref, _lists = {}, {}


def _reference(sort_limit):
    """clrrt_nn_batch(BATCH) of the fresh samples over the grown tree (default options), once per sort_limit."""
    if sort_limit not in _ref:
        pl = _grown({}, sort_limit)
        try:
            ids, keys = pl.sort_nodes_batch(list(_fresh_samples(pl)), exact=False)
            _ref[sort_limit] = (pl.size()[0], bytes(pl.nodes_raw()), ids, keys)
        finally:
            pl.close()
    return _ref[sort_limit]


def _partition_lists(cfg):
    """Part lists and merged lists of every partition under an option set, once per set."""
    if cfg not in _lists:
        pl = _grown(CONFIGS[cfg])
        try:
            N = pl.size()[0]
            assert bytes(pl.nodes_raw()) == _reference(10)[1]  # options never change the tree
            smp = _fresh_samples(pl)
            out = {}
            pl.reset_counters()
            for name, ranges in _partitions(N).items():
                parts = [pl.nn_range(smp, f, c) for f, c in ranges]
                stack = [np.stack([q[i] for q in parts]) for i in range(3)]
                out[name] = (ranges, parts, pl.nn_merge(*stack))
            w = pl.search_work()
            print(f"{cfg}: {N} nodes; walk tiles visited {w['tiles']}, exact keys {w['exact_keys']}, "
                  f"brute-force-equivalent keys {w['bf_keys']}, overflow records {pl.debug_counters()[32]}")
            assert w["bf_keys"] == NS * N * len(out) and w["samples"] == NS * sum(len(v[0]) for v in out.values())
            assert (w["tiles"] > 0) == (cfg != "brute")  # the range walk ran / did not run
            _lists[cfg] = (N, out)
        finally:
            pl.close()
    return _lists[cfg]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_part(ids, keys, cnt, first, count, sort_limit):
    assert ids.shape == (NS, K) and keys.shape == (NS, K) and cnt.shape == (NS,)
    assert (cnt >= 0).all() and (cnt <= min(sort_limit, count)).all()
    slot = np.arange(K)[None, :]
    used = slot < cnt[:, None]
    assert ((ids >= first) & (ids < first + count))[used].all()  # the nodes' own ids, inside the range
    assert (ids[~used] == -1).all() and np.isposinf(keys[~used]).all()
    # strictly ascending in (key bits, id): non-negative keys order as their bit patterns
    kb = _bits(keys).astype(np.int64)
    nxt = used[:, 1:]
    asc = (kb[:, 1:] > kb[:, :-1]) | ((kb[:, 1:] == kb[:, :-1]) & (ids[:, 1:] > ids[:, :-1]))
    assert asc[nxt].all()


def _check_merged(got, ref_ids, ref_keys):
    ids, keys, cnt = got
    ref_cnt = (ref_ids >= 0).sum(axis=1)
    assert np.array_equal(cnt, ref_cnt)
    assert np.array_equal(ids, ref_ids)  # all 10 slots (-1 past the count)
    used = np.arange(K)[None, :] < cnt[:, None]
    assert np.array_equal(_bits(keys)[used], _bits(ref_keys)[used])


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_partition_lists_equal_whole_tree_search(cfg):
    N, out = _partition_lists(cfg)
    Nr, _, ref_ids, ref_keys = _reference(10)
    print(f"{cfg}: tree of {N} nodes, {NS} samples, partitions {list(out)}")
    assert N == Nr and N > 2048  # ranges span more than one 1024-node super-tile
    assert (ref_ids >= 0).sum() > 5 * NS
    for name, (ranges, parts, merged) in out.items():
        assert sum(c for _, c in ranges) == N
        for (first, count), (ids, keys, cnt) in zip(ranges, parts):
            _check_part(ids, keys, cnt, first, count, 10)
        _check_merged(merged, ref_ids, ref_keys)
    if cfg != "brute":  # the walk's part lists against the brute force's over the same ranges
        _, bf = _partition_lists("brute")
        for name, (ranges, parts, _) in out.items():
            for (ids, keys, cnt), (bi, bk, bc) in zip(parts, bf[name][1]):
                assert np.array_equal(ids, bi) and np.array_equal(cnt, bc), name
                assert np.array_equal(_bits(keys), _bits(bk)), name


def test_sort_limit_below_ten():
    pl = _grown(CONFIGS["walk"], sort_limit=4)
    try:
        N, raw, ref_ids, ref_keys = _reference(4)
        assert pl.size()[0] == N and bytes(pl.nodes_raw()) == raw
        assert ((ref_ids >= 0).sum(axis=1) <= 4).all() and ((ref_ids >= 0).sum(axis=1) == 4).any()
        smp = _fresh_samples(pl)
        ranges = [cdist.node_range(N, 3, r) for r in range(3)]
        parts = [pl.nn_range(smp, f, c) for f, c in ranges]
        for (first, count), (ids, keys, cnt) in zip(ranges, parts):
            _check_part(ids, keys, cnt, first, count, 4)
        _check_merged(pl.nn_merge(*[np.stack([q[i] for q in parts]) for i in range(3)]), ref_ids, ref_keys)
    finally:
        pl.close()


def test_list_fed_rounds_grow_the_same_tree():
    """4 rounds x 1024 samples: clrrt_round_eval against nn_range over 3 node ranges + nn_merge +
    clrrt_round_eval_lists.  The first round's ranges over the lone root are empty or below the walk's minimum."""
    import torch
    B, rounds = 1024, 4
    buf = torch.zeros(2 * B * 160, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    trees = []
    for fed in (False, True):
        pl = _planner(dict(nn_walk_min=64), max_batch=B)
        try:
            rng = clrrt.Rng(SEED)
            for _ in range(rounds):
                smp = rng.draw_samples(pl.params, B)
                if fed:
                    N = pl.size()[0]
                    parts = [pl.nn_range(smp, *cdist.node_range(N, 3, r)) for r in range(3)]
                    ids, keys, cnt = pl.nn_merge(*[np.stack([q[i] for q in parts]) for i in range(3)])
                    n = pl.round_eval_lists(smp, ids, keys, cnt, buf.data_ptr())
                else:
                    n = pl.round_eval(smp, buf.data_ptr())
                pl.round_commit(buf.data_ptr(), n, 0, n)
            pl.rows_flush()
            nn, nr = pl.size()
            trees.append((nn, bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), pl.counters()))
        finally:
            pl.close()
    print(f"{rounds} rounds x {B}: {trees[0][0]} nodes, counters {trees[0][3]}")
    assert trees[0][0] > B
    assert trees[1][0] == trees[0][0]
    assert trees[1][1] == trees[0][1]  # node records
    assert trees[1][2] == trees[0][2]  # every trajectory row
    assert trees[1][3] == trees[0][3]


def _rc(err):
    return int(re.search(r"-> (-?\d+)", str(err.value)).group(1))


def test_argument_checks():
    EINVAL, ECAPACITY = -1, -3
    B = 256
    pl = _planner({}, max_nodes=1 << 16, max_batch=B)  # the allocation holds far more nodes than the tree
    try:
        pl.expand(clrrt.Rng(SEED), n_iters=2 * B, mode=clrrt.CLRRT_MODE_BATCH, batch=B)
        N = pl.size()[0]
        assert 16 < N < 1 << 12
        smp = clrrt.Rng(77).draw_samples(pl.params, B)
        big = clrrt.Rng(78).draw_samples(pl.params, B + 1)
        none = (abi.Sample * 0)()
        ids, keys, cnt = pl.nn_range(smp, 0, N)
        L, h = pl.L, pl.h
        vp = lambda a: a.ctypes.data  # noqa: E731
        n_out = C.c_int32(-7)
        # node ranges
        for first, count in ((-1, 2), (0, -1), (0, N + 1), (N, 1), (N + 1, 0), (1 << 40, 1)):
            with pytest.raises(clrrt.ClrrtError) as e:
                pl.nn_range(smp, first, count)
            assert _rc(e) == EINVAL, (first, count)
        assert (pl.nn_range(smp, N, 0)[2] == 0).all()  # an empty range at the end is a range
        # parts < 1
        for parts in (0, -2):
            with pytest.raises(clrrt.ClrrtError) as e:
                pl.nn_merge(vp(ids), vp(keys), vp(cnt), n=B, parts=parts)
            assert _rc(e) == EINVAL
        # null pointers with n > 0
        outs = (ids.copy(), keys.copy(), cnt.copy())  # kept alive: the valid call below writes them
        o = tuple(vp(a) for a in outs)
        assert L.clrrt_nn_range(h, None, B, 0, N, *o) == EINVAL
        assert L.clrrt_nn_merge(h, B, 1, vp(ids), vp(keys), vp(cnt), *o) == 0  # one part: the same lists
        assert np.array_equal(outs[0], ids) and np.array_equal(outs[2], cnt)
        assert L.clrrt_round_eval_lists(h, None, B, vp(ids), vp(keys), vp(cnt), None, C.byref(n_out)) == EINVAL
        assert L.clrrt_round_eval_lists(h, smp, B, vp(ids), vp(keys), vp(cnt), None, None) == EINVAL
        for q in range(3):
            a = [vp(ids), vp(keys), vp(cnt)]
            a[q] = None
            assert L.clrrt_nn_range(h, smp, B, 0, N, *a) == EINVAL
            assert L.clrrt_nn_merge(h, B, 1, *a, *o) == EINVAL
            assert L.clrrt_nn_merge(h, B, 1, vp(ids), vp(keys), vp(cnt), *[None if i == q else o[i] for i in range(3)]) == EINVAL
            assert L.clrrt_round_eval_lists(h, smp, B, *a, None, C.byref(n_out)) == EINVAL
        # more samples than max_batch
        wide = [np.zeros((B + 1, K), np.int32), np.zeros((B + 1, K), np.float32), np.zeros(B + 1, np.int32)]
        with pytest.raises(clrrt.ClrrtError) as e:
            pl.nn_range(big, 0, N)
        assert _rc(e) == ECAPACITY
        with pytest.raises(clrrt.ClrrtError) as e:
            pl.nn_merge(*[w[None] for w in wide])
        assert _rc(e) == ECAPACITY
        with pytest.raises(clrrt.ClrrtError) as e:
            pl.round_eval_lists(big, *wide, 0)
        assert _rc(e) == ECAPACITY
        # n == 0: OK, nothing happens
        assert L.clrrt_nn_range(h, none, 0, 0, N, None, None, None) == 0
        assert L.clrrt_nn_merge(h, 0, 1, None, None, None, None, None, None) == 0
        assert L.clrrt_round_eval_lists(h, none, 0, None, None, None, None, C.byref(n_out)) == 0 and n_out.value == 0
        # list validation, on the device before any rollout: counts in [0, sort_limit], ids in [0, tree size).  The
        # id N is outside the tree and inside the allocation.
        import torch
        buf = torch.zeros(2 * B * 160, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        before = (pl.size(), pl.counters(), bytes(pl.nodes_raw()))
        assert cnt[5] >= 1
        bad = []
        x = ids.copy(); x[5, 0] = N; bad.append((x, cnt, 5))
        x = ids.copy(); x[200, cnt[200] - 1 if cnt[200] else 0] = -1; c = cnt.copy(); c[200] = max(1, c[200])
        bad.append((x, c, 200))
        c = cnt.copy(); c[7] = 11; c[9] = -1; bad.append((ids, c, 7))
        c = cnt.copy(); c[255] = -1; bad.append((ids, c, 255))
        for bi, bc, who in bad:
            with pytest.raises(clrrt.ClrrtError, match=rf"sample {who}\b") as e:
                pl.round_eval_lists(smp, bi, keys, bc, buf.data_ptr())
            assert _rc(e) == EINVAL
            assert (pl.size(), pl.counters(), bytes(pl.nodes_raw())) == before
        n = pl.round_eval_lists(smp, ids, keys, cnt, buf.data_ptr())  # a valid call still works
        assert n > 0 and pl.counters()["rollouts"] > before[1]["rollouts"]
        pl.round_commit(buf.data_ptr(), n, 0, n)
        assert pl.size()[0] == N + n
    finally:
        pl.close()


# --- ranks over gloo on GPU 0, in the manner of tests/test_dist_gpu.py ------------------------------------------
HDR = 148  # clrrt_node bytes before owner / row_offset
RANK_CASES = [(2, 4096, 4), (4, 4099, 3)]  # (ranks, samples per round, rounds); 4099: uneven slices and ranges


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_planner(G):
    return _planner(dict(nn_walk_min=64), max_nodes=1 << 16, max_rows=1 << 25, max_batch=G)


def _rank_worker(rank, port, out_dir, world, G, rounds):
    sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    # a finite timeout: a rank whose peer died leaves its collective with an error instead of waiting
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    pl = _rank_planner(G)
    pl.set_rank(rank)
    pl.set_stream(torch.cuda.current_stream().cuda_stream)
    ps = cdist.PartitionedSearch(pl, G, "cuda")
    rx = cdist.RoundExchange(2 * G, "cuda", first_bound=G)
    rng = clrrt.Rng(SEED)
    for _ in range(rounds):
        n_local = ps.round_eval(rng.draw_samples(pl.params, G), rx.records_ptr())
        cat, counts, my_first, _ = rx.exchange(n_local, 0.0)
        pl.round_commit(cat.data_ptr() if cat.shape[0] else 0, cat.shape[0], my_first, counts[rank])
    raw = np.frombuffer(bytes(pl.nodes_raw()), dtype=np.uint8).reshape(-1, 160)
    g = pl.nodes()
    own = np.nonzero(g["owner"] == rank)[0]
    rows = [pl.rows(int(g["row_offset"][i]), int(g["nrows"][i])) for i in own]
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), hdr=raw[:, :HDR], own=own,
             rows=np.concatenate(rows) if rows else np.zeros((0, 10)), collectives=ps.collectives)
    dist.barrier()
    dist.destroy_process_group()
    pl.close()


@pytest.mark.parametrize("world,G,rounds", RANK_CASES)
def test_partitioned_ranks_match_single_process(tmp_path, world, G, rounds):
    """Every rank's tree equals ONE process's expand(BATCH, batch=G): headers bit for bit (owner and row_offset
    aside), each node's rows on its owner.  (A worker that raises ends the whole spawn: join=True.)"""
    import torch.multiprocessing as mp
    mp.spawn(_rank_worker, args=(_free_port(), str(tmp_path), world, G, rounds), nprocs=world, join=True)
    pl = _rank_planner(G)
    try:
        st = pl.expand(clrrt.Rng(SEED), n_iters=rounds * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
        assert st["rounds"] == rounds
        ref = np.frombuffer(bytes(pl.nodes_raw()), dtype=np.uint8).reshape(-1, 160)
        g = pl.nodes()
        ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
        print(f"{world} ranks, G = {G}, {rounds} rounds: {ref.shape[0]} nodes; owned {[len(r['own']) for r in ranks]}")
        assert ref.shape[0] > G
        for r in ranks:
            assert int(r["collectives"]) == rounds  # one all-gather of lists per round
            assert np.array_equal(r["hdr"], ref[:, :HDR])
        assert sum(len(r["own"]) for r in ranks) == ref.shape[0]
        for rk, r in enumerate(ranks):
            want = [pl.rows(int(g["row_offset"][i]), int(g["nrows"][i])) for i in r["own"]]
            want = np.concatenate(want) if want else np.zeros((0, 10))
            assert np.array_equal(r["rows"].view(np.uint64), want.view(np.uint64)), rk
    finally:
        pl.close()
