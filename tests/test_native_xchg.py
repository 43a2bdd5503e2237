"""The native exchange of the sharded expansion (include/clrrt_xchg.h, libclrrt_xchg.so) through a native program linked
against it and libclrrt (tests/native/xchg_shards.cpp), no Python in the rounds: W host threads with one context each
over the in-process transport, one rank over a one-rank RCCL communicator (option shard_hook_world1), the collective
failure and the missing-peer deadline, and k_xchg_concat against a host loop.  Every case compares with ONE unsharded
context in the same program: headers (148 bytes) bit for bit on every rank, each node's rows on its owner, iterations,
goal nodes, deferred samples; the program prints one line per case and "failures N".

The last test binds the same RCCL transport from Python (clrrt.dist.NativeExchange) with a world of one."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from clrrt import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "xchg_shards")


def test_xchg_shards_program_compiles_against_the_header():
    """CPU: the program compiles against clrrt_xchg.h (host C++ only)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "xchg_shards.cpp")], check=True)


def _run(tmp_path, *args):
    assert os.path.exists(EXE), "tests/native/xchg_shards not built (make -C cl-rrt_amd/csrc)"
    obs_path = tmp_path / "obs.bin"
    obs_path.write_bytes(np.ascontiguousarray(scenes.urban_scene(200), dtype="<f8").tobytes())
    r = subprocess.run([EXE, args[0], str(obs_path), *args[1:]], capture_output=True, text=True, timeout=240)
    print(r.stdout)
    print(r.stderr[-2000:])
    return r


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_concat_kernel_matches_host_loop(tmp_path):
    r = _run(tmp_path, "concat")
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 6


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_local_transport_matches_unsharded(tmp_path, case):
    """(W, G, defer_steps, nn_lag, rounds, first bound): 0 (2, 2048, 0, 1, 4, slice), 1 (3, 3065, 48, 1, 4, slice),
    2 (2, 2048, 64, 2, 6, slice), 3 (2, 2048, 0, 1, 4, 8: second gathers)."""
    r = _run(tmp_path, "local", str(case))
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 1


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_rccl_one_rank_matches_unsharded(tmp_path):
    r = _run(tmp_path, "rccl1")
    if "skipped rccl1" in r.stdout:
        pytest.skip("rccl1: " + [ln for ln in r.stdout.splitlines() if "SKIPPED" in ln][0])
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 1


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_failure_is_collective_and_missing_peer_times_out(tmp_path):
    r = _run(tmp_path, "failure")
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 2


def _native_worker(rank, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=1)
    import clrrt
    from clrrt import abi
    from clrrt import dist as cdist
    G, T, rounds = 1024, 48, 8
    raws = []
    for native in (True, False):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=abi.CLRRT_COLLISION_OBB), device=0, max_nodes=1 << 17,
                           max_rows=1 << 24, max_batch=G)
        pl.set_obstacles(scenes.urban_scene(200))
        pl.tree_init()
        pl.set_option("defer_steps", T)
        pl.set_option("nn_lag", 1)
        ex = None
        if native:
            pl.set_option("shard_hook_world1", 1)
            ex = cdist.NativeExchange(pl, cdist.exchange_capacity(G, T), "cuda:0", slice_size=G)
        st = pl.expand(clrrt.Rng(17), n_iters=rounds * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
        hdr = np.frombuffer(bytes(pl.nodes_raw()), dtype=np.uint8).reshape(-1, 160)[:, :148]  # before owner / row_offset
        raws.append((hdr.tobytes(), st["goal_nodes_added"], st["deferred"], ex.stats() if ex else None))
        if ex:
            ex.close()
        pl.close()
    np.savez(os.path.join(out_dir, "native.npz"), same=raws[0][:3] == raws[1][:3], nodes=len(raws[0][0]) // 148,
             exchanges=raws[0][3]["exchanges"], closing=raws[0][3]["closing"], collectives=raws[0][3]["collectives"])
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_python_native_exchange_one_rank(tmp_path):
    """clrrt.dist.NativeExchange (ctypes binding of the RCCL transport) with a world of one and shard_hook_world1: the
    tree, goal nodes and deferred samples equal the same planner's without a hook; rounds + 1 exchanges at least."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_native_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    r = np.load(tmp_path / "native.npz")
    print(f"NativeExchange world 1: {int(r['nodes'])} nodes, exchanges {int(r['exchanges'])}, collectives "
          f"{int(r['collectives'])}, closing {int(r['closing'])}")
    assert bool(r["same"]) and int(r["nodes"]) > 2000
    assert int(r["exchanges"]) >= 9 and int(r["closing"]) == 1 and int(r["collectives"]) == int(r["exchanges"])
