"""Sharded 5 Hz replanning without Python in the loop (tests/native/xchg_replan.cpp): the adapter's
MotionPlanner::planMotion on W ranks over the native exchange (include/clrrt_xchg.h), whose path completion
(clrrt_xchg_path_rows, k_xchg_path_select) gives every rank the committed path's rows that other ranks grew, against
ONE unsharded MotionPlanner in the same program: per query and rank the re-init outcome, iterations, tree size, every
header's first 148 bytes, the path ids, the committed path's rows bit for bit after the completion and the
CAR_TO_WORLD transform, and the filtered MPC message bit for bit.  The query inputs (pose, car-frame goal, obstacles)
come from the CPU oracle running the same sequence, and the unsharded program's path ids and message are compared
with the oracle's.  Also: the selection kernel against a host loop, the disagreement of the ranks' paths
(CLRRT_ESTATE on every rank, at once), a sharded query without a completer (the adapter throws), a one-rank RCCL
communicator, and clrrt.dist.NativeExchange.path_rows from Python with a world of one."""
import os
import socket
import struct
import subprocess
import sys

import numpy as np
import pytest

from clrrt import abi, replan, scenes
from oracle_binding import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "xchg_replan")
GOAL_W = (20.0, 0.0, 0.0, 0.0)
SEED, NQ, V0 = 11, 4, 1.0
MODE = abi.CLRRT_COLLISION_OBB

# (W, G, rounds per query, defer_steps, nn_lag)
CASES = [(2, 256, 2, 0, 1), (3, 3065, 3, 48, 1), (2, 2048, 3, 64, 2), (4, 1024, 3, 48, 1)]

_sequences = {}


def test_xchg_replan_program_compiles_against_the_headers():
    """CPU: the program compiles against clrrt_adapter.hpp and clrrt_xchg.h (host C++ only)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "xchg_replan.cpp")], check=True)


def test_path_entry_points_are_exported_and_reject_bad_arguments():
    """CPU: the library exports the completion's entry points, libclrrt exports clrrt_path_device, and null or
    out-of-range arguments are CLRRT_EINVAL before any device call."""
    import ctypes as C
    import clrrt
    from clrrt import dist as cdist
    libx = os.path.join(ROOT, "cl-rrt_amd", "libclrrt_xchg.so")
    out = subprocess.run(["nm", "-D", "--defined-only", libx], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"clrrt_xchg_path_rows", "clrrt_xchg_path_stats", "clrrt_xchg_selftest_path_select"} <= have
    assert "clrrt_path_device" in clrrt.exported_symbols()
    assert clrrt.lib().clrrt_path_device(None, None, None, None, None) == -1
    L = cdist.xchg_lib()
    moved = C.c_int64(7)
    assert L.clrrt_xchg_path_rows(None, None, C.byref(moved)) == -1 and moved.value == 0
    assert b"null" in L.clrrt_xchg_last_error()
    assert L.clrrt_xchg_path_stats(None, (C.c_int64 * 4)()) == -1
    one = (C.c_int32 * 1)(0)
    rows = (C.c_double * 10)()
    for W, me, n, owner, nrows in ((0, 0, 1, 0, 1), (65, 0, 1, 0, 1), (2, 2, 1, 0, 1), (2, -1, 1, 0, 1), (2, 0, -1, 0, 1),
                                   (2, 0, 1, 2, 1), (2, 0, 1, 0, 0)):
        assert L.clrrt_xchg_selftest_path_select(0, W, me, n, (C.c_int32 * 1)(owner), (C.c_int32 * 1)(nrows), rows,
                                                 C.byref(moved)) == -1, (W, me, n, owner, nrows)
    assert L.clrrt_xchg_selftest_path_select(0, 2, 0, 1, one, (C.c_int32 * 1)(1), rows, None) == -1


def _oracle_sequence(G, rounds, T):
    """The 4-query sequence on the oracle (computed once per (G, rounds, T)): per-query inputs and expected outputs."""
    key = (G, rounds, T)
    if key in _sequences:
        return _sequences[key]
    obs_world = scenes.urban_scene(200, 20)
    make = replan.default_make_params(MODE)
    o = Oracle(abi.default_params(collision_mode=MODE), None)
    Oracle.srand(SEED)
    pose = np.array([0.0, 0.0, 0.0, 0.0, V0, 0.0])
    inputs, want = [], []
    for q in range(NQ):
        goal_c = replan.goal_in_car_frame(GOAL_W, pose)
        obs_c = replan.obstacles_in_car_frame(obs_world, q * replan.QUERY_PERIOD, pose)
        inputs.append((pose.copy(), goal_c, obs_c))
        o.set_params(make(pose[4], goal_c))
        o.set_obstacles(obs_c)
        o.path_transform(False, pose)
        oc = o.initialize_tree([0.0, 0.0, 0.0, pose[3], pose[4], pose[5]])
        kept = o.size()
        ndef = o.expand_batch(G * rounds, G, stable=True, defer_steps=T, threads=16)
        n = o.size()
        ids = o.extract_best_path()
        o.path_commit(ids)
        o.path_transform(True, pose)
        msg = o.path_mpc_message(True)
        rows = np.concatenate([o.path_rows(i) for i in range(len(ids))]) if ids else np.zeros((0, 10))
        want.append(dict(outcome=oc, kept=kept, tree=n, ids=list(ids), msg=msg, deferred=ndef, rows=len(rows)))
        pose = replan.advance_pose(pose, rows)
    _sequences[key] = (inputs, want)
    return _sequences[key]


def _write_inputs(path, inputs):
    with open(path, "wb") as f:
        f.write(b"CLPM" + struct.pack("<ii", MODE, len(inputs)))
        for pose, goal_c, obs_c in inputs:
            f.write(np.asarray(pose, dtype="<f8").tobytes() + np.asarray(goal_c, dtype="<f8").tobytes())
            f.write(struct.pack("<i", len(obs_c)) + np.ascontiguousarray(obs_c, dtype="<f8").tobytes())


def _read_outputs(path):
    b = open(path, "rb").read()
    assert b[:4] == b"CLPO"
    off = 4

    def take(fmt):
        nonlocal off
        v = struct.unpack_from("<" + fmt, b, off)
        off += struct.calcsize("<" + fmt)
        return v

    out = []
    for _ in range(take("i")[0]):
        found, outcome, iterations, tree = take("iiqq")
        ids = list(take(f"{take('i')[0]}i"))
        published, m = take("ii")
        msg = np.frombuffer(b, dtype="<f8", count=7 * m, offset=off).reshape(m, 7)
        off += 56 * m
        take("4q")  # the fail counters
        assert take("i")[0] == 0  # no markers
        deferred, rows = take("qq")
        out.append(dict(found=found, outcome=outcome, iterations=iterations, tree=tree, ids=ids, published=published,
                        msg=msg, deferred=deferred, rows=rows))
    return out


def _check_scenario(want, T):
    """The conditions that keep the comparison from passing over nothing, on the oracle's sequence."""
    for q, w in enumerate(want):
        assert 3 <= len(w["ids"]) <= 5 and 162 <= w["rows"] <= 166, (q, w["ids"], w["rows"])
        assert w["ids"][-1] >= w["kept"], (q, "no node of the path was grown in this query", w["ids"], w["kept"])
        assert w["outcome"] == (abi.REINIT_EMPTY if q == 0 else abi.REINIT_KEPT), (q, w["outcome"])
        if T > 0:
            assert w["deferred"] > 0, q


def _run(*args, timeout=240):
    assert os.path.exists(EXE), "tests/native/xchg_replan not built (make -C cl-rrt_amd/csrc)"
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    print(r.stderr[-2000:])
    return r


def _inputs_file(tmp_path, G, rounds, T):
    inputs, want = _oracle_sequence(G, rounds, T)
    fin = tmp_path / "in.bin"
    _write_inputs(fin, inputs)
    return fin, want


@pytest.mark.parametrize("case", CASES)
def test_oracle_scenario_exercises_the_completion(case):
    """CPU: on the oracle every query commits a path of 3-5 nodes and 162-166 rows with a node grown in that query,
    queries 1-3 re-initialise with outcome KEPT, and the T > 0 cases defer samples in every query."""
    _, G, rounds, T, _ = case
    _check_scenario(_oracle_sequence(G, rounds, T)[1], T)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_select_kernel_matches_host_loop():
    r = _run("select")
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 9


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", CASES)
def test_sharded_replanning_matches_unsharded(tmp_path, case):
    W, G, rounds, T, lag = case
    fin, want = _inputs_file(tmp_path, G, rounds, T)
    _check_scenario(want, T)
    fout = tmp_path / "out.bin"
    r = _run("local", fin, fout, W, G, rounds, T, lag)
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 1
    # the unsharded program against the oracle (code the parent commit has too)
    got = _read_outputs(fout)
    assert len(got) == NQ
    for q, (g, w) in enumerate(zip(got, want)):
        assert g["outcome"] == w["outcome"] and g["iterations"] == G * rounds and g["tree"] == w["tree"], q
        assert g["ids"] == w["ids"] and g["found"] == 1 and g["rows"] == w["rows"], q
        assert g["deferred"] == w["deferred"], q
        wm = np.delete(w["msg"], 3, axis=1)  # the adapter's message drops delta
        assert g["msg"].shape == wm.shape, q
        assert np.array_equal(g["msg"].view(np.uint64), np.ascontiguousarray(wm).view(np.uint64)), q


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_path_mismatch_is_estate_on_every_rank(tmp_path):
    fin, _ = _inputs_file(tmp_path, 256, 2, 0)
    r = _run("mismatch", fin, 256, 2)
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 1


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_query_without_completer_throws(tmp_path):
    fin, _ = _inputs_file(tmp_path, 256, 2, 0)
    r = _run("nocompleter", fin, 256, 2)
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 1


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_rccl_one_rank_completion_matches_unsharded(tmp_path):
    fin, _ = _inputs_file(tmp_path, 1024, 3, 48)
    r = _run("rccl1", fin, 1024, 3, 48, 1)
    if "skipped rccl1" in r.stdout:
        pytest.skip("rccl1: " + [ln for ln in r.stdout.splitlines() if "SKIPPED" in ln][0])
    assert r.returncode == 0 and "failures 0" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 1


def _native_worker(rank, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=1)
    import clrrt
    from clrrt import dist as cdist
    G = 256
    pl = clrrt.Planner(clrrt.default_params(goal=GOAL_W, collision_mode=MODE), device=0, max_nodes=1 << 16,
                       max_rows=1 << 21, max_batch=G)
    pl.set_obstacles(scenes.urban_scene(200))
    pl.tree_init()
    pl.set_option("shard_hook_world1", 1)
    ex = cdist.NativeExchange(pl, cdist.exchange_capacity(G, 0), "cuda:0", slice_size=G)
    pl.expand(clrrt.Rng(SEED), n_iters=4 * G, mode=clrrt.CLRRT_MODE_BATCH, batch=G)
    ids, _, _ = pl.extract_best_path()
    pl.path_commit(ids)
    nodes0, rows0 = pl.path_download()
    moved = ex.path_rows(pl)
    nodes1, rows1 = pl.path_download()
    st = ex.path_stats()
    np.savez(os.path.join(out_dir, "path.npz"), moved=moved, n=len(ids), rows=len(rows0),
             same=bytes(nodes0) == bytes(nodes1) and rows0.tobytes() == rows1.tobytes(),
             completions=st["completions"], collectives=st["collectives"], taken=st["rows_taken"])
    ex.close()
    pl.close()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_python_native_exchange_path_rows_one_rank(tmp_path):
    """clrrt.dist.NativeExchange.path_rows with a world of one: 0 rows moved, the downloaded path unchanged."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_native_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    r = np.load(tmp_path / "path.npz")
    print(f"NativeExchange.path_rows world 1: path {int(r['n'])} nodes, {int(r['rows'])} rows, moved {int(r['moved'])}, "
          f"collectives {int(r['collectives'])}")
    assert int(r["n"]) >= 2 and int(r["rows"]) > 0, "no path: the comparison covers nothing"
    assert int(r["moved"]) == 0 and int(r["taken"]) == 0 and bool(r["same"])
    assert int(r["completions"]) == 1 and int(r["collectives"]) >= 1
