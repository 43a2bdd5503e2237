"""The lag-2 rounds' appended-node search as a walk over the appended range's own index (option nn_delta_walk,
launch_nn_delta_walk in clrrt_nnwalk.hip) -- GPU.

* List level (option nn_delta_verify): every appended-node walk is followed by the brute force (k_nn_partial) over
  the same range and key caps, and a device kernel compares, per sample, all NN_K (key bits, id) pairs of the two
  partial-list sets; work counters 38 / 39 = samples compared / differing.
* Tree level: the shapes at which the index or the walk can go wrong grow, byte for byte, the tree of unpipelined
  rounds (nn_pipeline 0), as tests/test_gpu_parity.py::test_pipelined_batch_rounds_identical checks at full size.
* Sharded: two ranks on GPU 0 (gloo), each searching its slice of the round's samples, grow the single-process tree.
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


def _plain_tree(batch, rounds, defer=0):
    """The unpipelined rounds' tree of a shape, grown once."""
    key = (batch, rounds, defer)
    if key not in _plain:
        _plain[key] = _grow(dict(nn_pipeline=0, defer_steps=defer), batch, rounds)[:3]
    return _plain[key]


@pytest.mark.parametrize("defer", [0, 16])
def test_partial_lists_equal_brute_force(defer):
    """8 rounds of 512 samples from a fresh tree (the first rounds are full of the root's zero-length children: the
    runs of equal records), the walk served from 64 nodes on: every appended-node walk's lists equal the brute
    force's, all NN_K ids and key bit patterns of every sample."""
    opts = dict(nn_walk_min=64, nn_lag=2, nn_delta_verify=1, defer_steps=defer)
    raw, rows, n, d = _grow(opts, 512, 8)
    print(f"defer_steps {defer}: {n} nodes; samples compared {d[38]}, differing {d[39]}; walk per sample: tiles "
          f"{d[41] / max(1, d[38]):.1f}, prefiltered in {d[42] / max(1, d[38]):.1f}, exact keys {d[43] / max(1, d[38]):.1f}; "
          f"brute force queued {d[54] / max(1, d[38]):.1f}, exact keys {d[55] / max(1, d[38]):.1f}")
    assert d[38] > 0
    assert d[39] == 0
    assert (raw, rows, n) == _plain_tree(512, 8, defer)


SHAPES = [
    # batch 96: appended ranges below one tile and no multiples of 32 or 1024 (the shortest take the brute force)
    (96, 8, dict()),
    (96, 8, dict(nn_delta_walk=0)),
    # batch 2048 x 5 rounds: more than one super-tile per range
    (2048, 5, dict()),
    (2048, 5, dict(nn_delta_walk=0)),
    # every sample overflows its walk: the caps come from k_walk_seed_ovf
    (2048, 5, dict(nn_walk_budget_tiles=1, nn_walk_budget_keys=1)),
    (96, 8, dict(nn_walk_budget_tiles=1, nn_walk_budget_keys=1)),
]


@pytest.mark.parametrize("batch,rounds,extra", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_tree_identical_to_unpipelined_rounds(batch, rounds, extra):
    opts = dict(nn_walk_min=64, nn_lag=2)
    opts.update(extra)
    raw, rows, n, _ = _grow(opts, batch, rounds, max_rows=1 << 25 if batch > 512 else 1 << 23)
    want = _plain_tree(batch, rounds)
    print(f"batch {batch} x {rounds} {extra}: {n} nodes")
    assert n > batch // 2
    assert (raw, rows, n) == want


@pytest.mark.parametrize("walk", [1, 0])
def test_rounds_that_append_nothing(walk):
    """A box over the root: every rollout collides, no round appends a node (count == 0: no index, no search, no
    merge), and the pipeline still ends with the tree of unpipelined rounds."""
    wall = np.array([[0.0, 0.0, 0.0, 12.0, 12.0, 0.0, 0.0]])
    got = _grow(dict(nn_walk_min=0, nn_lag=2, nn_delta_walk=walk), 96, 5, obs=wall)
    want = _grow(dict(nn_pipeline=0), 96, 5, obs=wall)
    assert got[2] == 1, got[2]
    assert got[:3] == want[:3]


# --- sharded: two ranks on GPU 0 over gloo, in the manner of tests/test_dist_gpu.py -------------------------------
WORLD, G, ROUNDS = 2, 2 * 1024 - 6, 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_planner():
    pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), device=0, max_nodes=1 << 16,
                       max_rows=1 << 25, max_batch=G)
    pl.set_obstacles(scenes.urban_scene(200))
    pl.tree_init()
    pl.set_option("nn_walk_min", 64)
    pl.set_option("nn_lag", 2)
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
    np.savez(os.path.join(out_dir, f"shard{rank}.npz"), hdr=raw[:, :148], rounds=st["rounds"], ex_rounds=ex.rounds)
    dist.barrier()
    dist.destroy_process_group()
    pl.close()


def test_sharded_slices_match_single_process(tmp_path):
    """Each rank's appended-node walk searches its slice of the round's samples (A.n < the round's samples, uneven
    slices); both ranks' trees equal the single process's (headers: owner and row_offset aside)."""
    import torch.multiprocessing as mp
    mp.spawn(_shard_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    pl = _shard_planner()
    st = pl.expand(clrrt.Rng(SEED), n_iters=ROUNDS * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
    assert st["rounds"] == ROUNDS
    ref = np.frombuffer(bytes(pl.nodes_raw()), dtype=np.uint8).reshape(-1, 160)[:, :148]
    pl.close()
    assert ref.shape[0] > G
    for r in range(WORLD):
        got = np.load(tmp_path / f"shard{r}.npz")
        assert int(got["rounds"]) == ROUNDS
        assert np.array_equal(got["hdr"], ref)
