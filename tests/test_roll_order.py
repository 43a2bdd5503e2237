"""The rollout queue's order by predicted chain length (option roll_priority: k_roll_flag's length classes,
k_roll_order's stable partition, clrrt_kernels.hip) -- GPU.

* Tree level: the order is scheduling only, so roll_priority 1 grows, byte for byte (node records, trajectory rows,
  node count), the tree of roll_priority 0 -- on the default grid (queues this short keep the plain order) and on
  a grid of 2 blocks (served by class), with deferred samples off (defer_steps 0), with a cap below most class
  bounds (16: nearly every job in the top class) and at the benchmark's cap (128).
* Order level (option roll_order_verify): the order is built for every queue and a device kernel checks every
  round's perm: a permutation of [0, njobs), classes not increasing along the queue, q ascending within a class;
  work counters 6 / 7 = positions checked / wrong.
* Degenerate queues: 10 jobs (less than a wave), and a scene in which every job lands in one class.
* Sharded: two ranks on GPU 0 (gloo), each ordering its slice's jobs, grow the single-process tree.
"""
import os
import socket
import sys

import numpy as np
import pytest

import clrrt
from clrrt import abi, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12
BASE = dict(nn_walk_min=64, nn_lag=2)


def _grow(opts, batch, rounds, obs=None, max_nodes=1 << 15, max_rows=1 << 23):
    """One query of `rounds` BATCH rounds; (node records, trajectory rows, nodes, debug counters)."""
    if obs is None:
        obs = scenes.urban_scene(200)
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), max_nodes=max_nodes,
                       max_rows=max_rows, max_batch=batch)
    try:
        for k, v in opts.items():
            pl.set_option(k, v)
        pl.set_obstacles(obs)
        pl.tree_init()
        st = pl.expand(clrrt.Rng(SEED), n_iters=batch * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=batch)
        assert st["rounds"] == rounds, st
        n, nr = pl.size()
        return bytes(pl.nodes_raw()), pl.rows(0, nr).tobytes(), n, pl.debug_counters()
    finally:
        pl.close()


_plain = {}


def _plain_tree(batch, rounds, defer):
    """The tree of a shape under the plain queue order (roll_priority 0), grown once."""
    key = (batch, rounds, defer)
    if key not in _plain:
        _plain[key] = _grow(dict(BASE, roll_priority=0, defer_steps=defer), batch, rounds,
                            max_rows=1 << 25 if batch > 512 else 1 << 23)[:3]
    return _plain[key]


# batch 96 x 8 rounds: 960 jobs, no multiple of the order kernels' 256 positions per block, some classes empty;
# batch 2048 x 5 rounds: 80 blocks
SHAPES = [(96, 8), (2048, 5)]


# roll_blocks 0: the default grid, whose lanes hold these queues at once, so the round keeps the plain order (the
# fall-back); roll_blocks 2: 512 lanes, every queue here is longer and is served by class
@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("defer", [0, 16, 128])
@pytest.mark.parametrize("batch,rounds", SHAPES)
def test_tree_identical_to_plain_order(batch, rounds, defer, blocks):
    raw, rows, n, _ = _grow(dict(BASE, roll_priority=1, defer_steps=defer, roll_blocks=blocks), batch, rounds,
                            max_rows=1 << 25 if batch > 512 else 1 << 23)
    print(f"batch {batch} x {rounds}, defer_steps {defer}, roll_blocks {blocks}: {n} nodes")
    assert n > batch // 2
    assert (raw, rows, n) == _plain_tree(batch, rounds, defer)


@pytest.mark.parametrize("defer", [0, 16, 128])
@pytest.mark.parametrize("batch,rounds", SHAPES)
def test_order_is_a_stable_partition(batch, rounds, defer):
    raw, rows, n, d = _grow(dict(BASE, roll_priority=1, roll_order_verify=1, defer_steps=defer), batch, rounds,
                            max_rows=1 << 25 if batch > 512 else 1 << 23)
    print(f"batch {batch} x {rounds}, defer_steps {defer}: positions checked {d[6]}, wrong {d[7]}")
    assert d[6] > 0
    assert d[7] == 0
    assert (raw, rows, n) == _plain_tree(batch, rounds, defer)


def test_queue_shorter_than_a_wave():
    """Batch 1 x 4 rounds: 10 jobs."""
    got = _grow(dict(BASE, roll_priority=1, roll_order_verify=1, defer_steps=128), 1, 4)
    want = _grow(dict(BASE, roll_priority=0, defer_steps=128), 1, 4)
    assert got[3][6] > 0
    assert got[3][7] == 0
    assert got[:3] == want[:3]


def test_every_job_in_one_class():
    """A box over the root: the tree stays the root, so a sample's list holds the root at rest as candidate 0 (a
    first-half standing-start class) and no other candidate (class 0), and no round appends a node."""
    wall = np.array([[0.0, 0.0, 0.0, 12.0, 12.0, 0.0, 0.0]])
    got = _grow(dict(BASE, nn_walk_min=0, roll_priority=1, roll_order_verify=1, defer_steps=128), 96, 5, obs=wall)
    want = _grow(dict(BASE, nn_walk_min=0, roll_priority=0, defer_steps=128), 96, 5, obs=wall)
    assert got[2] == 1, got[2]
    assert got[3][6] > 0
    assert got[3][7] == 0
    assert got[:3] == want[:3]


# --- sharded: two ranks on GPU 0 over gloo, in the manner of tests/test_nn_delta_walk.py --------------------------
WORLD, G, ROUNDS = 2, 96, 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_planner():
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), device=0, max_nodes=1 << 15,
                       max_rows=1 << 23, max_batch=G)
    pl.set_obstacles(scenes.urban_scene(200))
    pl.tree_init()
    for k, v in BASE.items():
        pl.set_option(k, v)
    pl.set_option("roll_priority", 1)
    pl.set_option("roll_order_verify", 1)
    return pl


def _shard_worker(rank, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from clrrt import dist as cdist
    pl = _shard_planner()
    pl.set_stream(torch.cuda.current_stream().cuda_stream)
    ex = cdist.ShardExchange(pl, cdist.exchange_capacity(-(-G // WORLD), 0), "cuda", slice_size=-(-G // WORLD))
    st = pl.expand(clrrt.Rng(SEED), n_iters=ROUNDS * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
    raw = np.frombuffer(bytes(pl.nodes_raw()), dtype=np.uint8).reshape(-1, 160)
    d = pl.debug_counters()
    np.savez(os.path.join(out_dir, f"shard{rank}.npz"), hdr=raw[:, :148], rounds=st["rounds"], ex_rounds=ex.rounds,
             checked=d[6], wrong=d[7])
    dist.barrier()
    dist.destroy_process_group()
    pl.close()


def test_sharded_slices_match_single_process(tmp_path):
    """Each rank orders the jobs of its slice of the round's samples (48 samples: 480 jobs); both ranks' trees equal
    the single process's (headers: owner and row_offset aside)."""
    import torch.multiprocessing as mp
    mp.spawn(_shard_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    pl = _shard_planner()
    pl.set_option("roll_priority", 0)
    st = pl.expand(clrrt.Rng(SEED), n_iters=ROUNDS * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
    assert st["rounds"] == ROUNDS
    ref = np.frombuffer(bytes(pl.nodes_raw()), dtype=np.uint8).reshape(-1, 160)[:, :148]
    pl.close()
    assert ref.shape[0] > G // 2
    for r in range(WORLD):
        got = np.load(tmp_path / f"shard{r}.npz")
        assert int(got["rounds"]) == ROUNDS
        assert int(got["checked"]) > 0
        assert int(got["wrong"]) == 0
        assert np.array_equal(got["hdr"], ref)
