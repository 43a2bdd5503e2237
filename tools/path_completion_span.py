"""Measurement (not a test): the host-staged completion of the committed path, clrrt.dist.fetch_path_rows, per query of
a sharded 5 Hz sequence -- two torch.distributed ranks (gloo) sharing GPU 0, clrrt.dist.ShardExchange in the rounds,
the scene and sequence of tests/test_native_xchg_replan.py (urban_scene(200, 20), goal 20 m ahead, v0 = 1, seed 11,
4 queries).  The figure is the host time from the call to its return (it ends in path_load, which waits for the
stream), the same bracket `tests/native/xchg_replan span` puts around the device-side completion
(clrrt_xchg_path_rows), so the two compare.  Each sequence runs twice; the second run is printed.

    python tools/path_completion_span.py [G rounds defer_steps nn_lag]        (default 2048 3 64 2)
"""
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2


def _worker(rank, port, G, rounds, T, lag):
    sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    import clrrt
    from clrrt import abi, replan, scenes
    from clrrt import dist as cdist
    mode = abi.CLRRT_COLLISION_OBB
    sl = -(-G // WORLD)
    for rep in range(2):
        pl = clrrt.Planner(clrrt.default_params(collision_mode=mode), device=0, max_nodes=1 << 16, max_rows=1 << 23,
                           max_batch=sl)
        pl.set_option("defer_steps", T)
        pl.set_option("nn_lag", lag)
        pl.set_stream(torch.cuda.current_stream().cuda_stream)
        ex = cdist.ShardExchange(pl, cdist.exchange_capacity(sl, T), "cuda", slice_size=sl)
        spans = []

        def complete(p):
            t0 = time.perf_counter()
            moved = cdist.fetch_path_rows(p, rank)
            spans.append((1e6 * (time.perf_counter() - t0), moved, p.path_size()))
            return moved

        rng = clrrt.Rng(11)
        backend = replan.PlannerBackend(pl, replan.default_make_params(mode), complete_path=complete)
        replan.run_queries(backend, lambda q: pl.expand(rng, n_iters=G * rounds, mode=clrrt.CLRRT_MODE_BATCH, batch=G),
                           4, scenes.urban_scene(200, 20), goal_world=(20.0, 0.0, 0.0, 0.0), v0=1.0)
        if rep == 1:
            for q, (us, moved, (n, rows)) in enumerate(spans):
                print(f"span fetch_path_rows gloo W={WORLD} G={G} rounds={rounds} T={T} lag={lag} rank {rank} query {q}: "
                      f"completion {us:.1f} us (path {n} nodes, {rows} rows, {moved} rows taken)", flush=True)
        dist.barrier()
        pl.close()
    dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    G, rounds, T, lag = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (2048, 3, 64, 2)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(port, G, rounds, T, lag), nprocs=WORLD, join=True)


if __name__ == "__main__":
    main()
