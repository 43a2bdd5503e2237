"""Multi-GPU round exchange: samples shard by rank, accepted-node records are
all-gathered after every round and appended by every rank in global sample order, so the trees stay
identical.  One process per GPU; backend "nccl" (RCCL over xGMI) on the GPU box, "gloo" in the CPU
tests.

Record = clrrt_node (160 bytes, include/clrrt.h); rank r holds the records of its contiguous slice of
the round's samples, in sample order, so concatenating the slices in rank order IS global order.
"""
import torch
import torch.distributed as dist

REC_BYTES = 160
GOAL_OFFSET = 140  # clrrt_node.goal (int32)


class RoundExchange:
    """All-gather of one round's accepted-node records, count-prefixed.

    Row 0 of `buf` is a header (int64 record count, float64 elapsed query ms, int64 aux value summed over the
    ranks, float64[4] bounds of the rank's record positions); clrrt_round_eval writes
    this rank's records from row 1 on (`records_ptr`).  One all-gather moves header + the first `bound`
    record rows of every rank, so no count exchange (and no host sync) precedes the data; the headers
    are read back once afterwards -- the one host wait of a round: the engine appends the union, so it needs the
    counts (and the budget word, the bounds) on the host.
    `bound` starts at `first_bound` (the sharded expansion passes this rank's slice size: a round commits
    about 0.4 records per sample) and adapts to 1.25x the largest count seen; a round whose count exceeds it
    (rare) moves the excess with a second all-gather (`second_gathers`; `collectives` counts them all).
    gloo (CPU rehearsal of the path) stages device buffers through the host.
    """

    HDR = 56

    def __init__(self, cap_records, device, group=None, first_bound=1024):
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.cap = int(cap_records)
        self.dev = torch.device(device)
        self.buf = torch.zeros((self.cap + 1, REC_BYTES), dtype=torch.uint8, device=self.dev)
        self.bound = min(self.cap, first_bound)
        self.host = dist.get_backend(group) == "gloo" and self.dev.type != "cpu"
        self.second_gathers = 0
        self.collectives = 0
        self.exchanges = 0

    def records_ptr(self):
        """Device address where this rank's clrrt_round_eval output goes (row 1 of the buffer)."""
        return self.buf.data_ptr() + REC_BYTES

    def records(self):
        return self.buf[1:]

    def _gather(self, t):
        self.collectives += 1
        src = t.cpu() if self.host else t.contiguous()
        parts = [torch.empty_like(src) for _ in range(self.world)]
        dist.all_gather(parts, src, group=self.group)
        return parts

    def exchange(self, n_local, elapsed_ms, aux=0, bbox=None, engine_stream=None):
        """Returns (records (total, 160) uint8 on the buffer's device in global sample order, counts
        per rank, first row of this rank's records, max elapsed ms over ranks); the sum of `aux` over the
        ranks is left in self.aux_sum and the union of the ranks' `bbox` (x0, y0, x1, y1) in self.bbox_all.

        engine_stream (a HIP stream handle): the stream the records were written on and the gathered records will
        be read on.  The gather is ordered after it and it after the gather by stream waits, not by the host;
        without one, torch's stream is synchronised before returning (the round API's callers)."""
        import numpy as np
        self.exchanges += 1
        cuda = self.dev.type == "cuda"
        ext = None
        if cuda and engine_stream:
            cur = torch.cuda.current_stream(self.dev)
            if int(engine_stream) != cur.cuda_stream:
                ext = torch.cuda.ExternalStream(int(engine_stream), device=self.dev)
                cur.wait_stream(ext)  # the records were written on the engine's stream
        hdr = np.zeros(self.HDR // 8, dtype=np.float64)
        hdr.view(np.int64)[0] = int(n_local)
        hdr[1] = float(elapsed_ms)
        hdr.view(np.int64)[2] = int(aux)
        hdr[3:7] = bbox if bbox is not None else (np.inf, np.inf, -np.inf, -np.inf)
        self.buf[0, :self.HDR].copy_(torch.from_numpy(hdr.view(np.uint8)))
        parts = self._gather(self.buf[:self.bound + 1])
        heads = torch.stack([q[0, :self.HDR] for q in parts]).cpu().numpy()
        counts = [int(c) for c in heads[:, :8].copy().view(np.int64)[:, 0]]
        t_max = float(heads[:, 8:16].copy().view(np.float64).max())
        self.aux_sum = int(heads[:, 16:24].copy().view(np.int64).sum())
        bb = heads[:, 24:56].copy().view(np.float64).reshape(-1, 4)
        self.bbox_all = (float(bb[:, 0].min()), float(bb[:, 1].min()), float(bb[:, 2].max()), float(bb[:, 3].max()))
        maxc = max(counts)
        extra = None
        if maxc > self.bound:
            # the excess rows of every rank (padded to the largest count) in a second collective
            self.second_gathers += 1
            extra = self._gather(self.buf[1 + self.bound:1 + maxc])
        pieces = []
        for r in range(self.world):
            c = counts[r]
            pieces.append(parts[r][1:1 + min(c, self.bound)])
            if c > self.bound:
                pieces.append(extra[r][:c - self.bound])
        self.bound = min(self.cap, max(self.bound, int(maxc * 1.25) + 64))
        total = sum(counts)
        cat = torch.cat(pieces, 0) if total else self.buf[1:1]
        if self.host and total:
            cat = cat.to(self.dev)
        cat = cat.contiguous()
        if cuda:
            if ext is not None:
                ext.wait_stream(torch.cuda.current_stream(self.dev))  # the engine reads the gathered records
            elif not engine_stream:
                # no engine stream named: the caller reads the records on a stream of its own choosing
                torch.cuda.current_stream(self.dev).synchronize()
        return cat, counts, sum(counts[:self.rank]), t_max


class ShardExchange:
    """The exchange hook of the engine's own sharded rounds (clrrt_set_shards): clrrt_expand runs every
    round -- this rank's slice of the samples, the lag-2 pipeline, deferred samples -- and calls back once
    per round with its records in `records_ptr()` (written on the engine's stream, which it does not wait for);
    the callback runs RoundExchange's count-prefixed all-gather (RCCL over xGMI with the nccl backend) ordered
    after the engine's stream by a stream wait, and hands the concatenation in rank order back, with the largest
    elapsed query time over the ranks (the engine's budget decision, identical on every rank) and the union of the
    ranks' position bounds; the engine's stream waits for the gather (no host synchronisation besides reading
    the headers).  Every sharded expansion ends with a closing exchange (no records) that carries any rank's
    failure.  One code path for 1 and N GPUs: with world 1 the engine appends its records itself."""

    def __init__(self, planner, cap_records, device, group=None, first_bound=None, slice_size=None):
        import traceback
        from . import EXCHANGE_FN
        if first_bound is None:
            # a round commits ~0.4 records per sample of the slice (2 at most): one slice's worth of rows covers the
            # first rounds without a second gather (then the bound follows the counts seen)
            first_bound = int(slice_size) + 64 if slice_size else 1024
        self.rx = RoundExchange(cap_records, device, group, first_bound)
        self.rank, self.world = self.rx.rank, self.rx.world
        self._keep = None
        self.rounds = 0
        self.closing = 0  # closing exchanges (one per sharded expansion)

        def cb(user, iop):
            try:
                io = iop.contents
                cat, counts, _, t_max = self.rx.exchange(io.n_local, io.elapsed_ms, io.aux_local,
                                                         tuple(io.bbox_local), io.stream or 0)
                self._keep = cat  # the engine reads it (stream-ordered) before the next exchange
                io.dev_all = cat.data_ptr() if cat.shape[0] else None
                io.n_all = int(cat.shape[0])
                io.max_elapsed_ms = float(t_max)
                io.aux_sum = self.rx.aux_sum
                for q in range(4):
                    io.bbox_all[q] = self.rx.bbox_all[q]
                self.rounds += 1
                self.closing += bool(io.flags & 1)
                return 0
            except Exception:  # reported to the engine, which returns CLRRT_EHIP
                traceback.print_exc()
                return -1

        self._cb = EXCHANGE_FN(cb)
        planner.set_shards(self.rank, self.world, self.rx.records_ptr(), self.rx.cap, self._cb)

    @property
    def second_gathers(self):
        return self.rx.second_gathers

    @property
    def collectives(self):
        """All-gathers issued (one per round unless a round's count passed the bound)."""
        return self.rx.collectives


_xlib = None


def xchg_lib():
    """libclrrt_xchg.so (include/clrrt_xchg.h), loaded after libclrrt.so (raises loudly when it has not been built)."""
    global _xlib
    if _xlib is None:
        import ctypes as C
        import os
        from . import EXCHANGE_FN, PKG_DIR, abi, lib
        lib()  # libclrrt.so first (and, through it, the one HIP runtime of the process)
        L = C.CDLL(os.path.join(PKG_DIR, "libclrrt_xchg.so"))
        P = C.POINTER
        sigs = {
            "clrrt_xchg_last_error": (C.c_char_p, []),
            "clrrt_xchg_unique_id": (C.c_int, [C.c_void_p]),
            "clrrt_xchg_create_rccl": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 P(C.c_void_p)]),
            "clrrt_xchg_group_create": (C.c_int, [C.c_int32, C.c_int32, P(C.c_void_p)]),
            "clrrt_xchg_group_destroy": (None, [C.c_void_p]),
            "clrrt_xchg_create_local": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                  P(C.c_void_p)]),
            "clrrt_xchg_hook": (C.c_int32, [C.c_void_p, P(abi.ExchangeIO)]),
            "clrrt_xchg_attach": (C.c_int, [C.c_void_p, C.c_void_p]),
            "clrrt_xchg_records": (C.c_void_p, [C.c_void_p]),
            "clrrt_xchg_stats": (C.c_int, [C.c_void_p, P(C.c_int64)]),
            "clrrt_xchg_destroy": (None, [C.c_void_p]),
            "clrrt_xchg_path_rows": (C.c_int32, [C.c_void_p, C.c_void_p, P(C.c_int64)]),
            "clrrt_xchg_path_stats": (C.c_int, [C.c_void_p, P(C.c_int64)]),
            "clrrt_xchg_selftest_path_select": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_int32),
                                                          P(C.c_int32), C.c_void_p, P(C.c_int64)]),
            "clrrt_xchg_selftest_concat": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, P(C.c_int32), P(C.c_double),
                                                     P(C.c_int64), P(C.c_double), C.c_int32, C.c_void_p, C.c_int64,
                                                     P(C.c_int64)]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _xlib = L
    return _xlib


UID_BYTES = 128  # CLRRT_XCHG_UID_BYTES


class NativeExchange:
    """ShardExchange's job without Python in the rounds: the hook is libclrrt_xchg's C function (clrrt_xchg_hook,
    include/clrrt_xchg.h) over its RCCL transport -- ncclAllGather on the engine's stream, k_xchg_concat, one read
    of the pinned summary -- so clrrt_expand calls no Python (and takes no GIL) per round.  One process per GPU; the
    process group only carries the communicator's unique id from its rank 0 to the others, once.  With a world of 1
    the planner keeps the hook only under its option "shard_hook_world1" (set it before constructing this)."""

    def __init__(self, planner, cap_records, device, group=None, first_bound=None, slice_size=None):
        import ctypes as C
        from . import ClrrtError
        L = xchg_lib()
        self.L = L
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        if first_bound is None:
            first_bound = int(slice_size) + 64 if slice_size else 1024  # as ShardExchange
        dev = torch.device(device)
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        uid = (C.c_ubyte * UID_BYTES)()
        if self.rank == 0 and L.clrrt_xchg_unique_id(uid) != 0:
            raise ClrrtError(f"clrrt_xchg_unique_id: {L.clrrt_xchg_last_error().decode()}")
        box = [bytes(uid)]
        if self.world > 1:
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        uid = (C.c_ubyte * UID_BYTES).from_buffer_copy(box[0])
        h = C.c_void_p()
        if L.clrrt_xchg_create_rccl(uid, self.rank, self.world, index, int(cap_records), int(first_bound),
                                    C.byref(h)) != 0:
            raise ClrrtError(f"clrrt_xchg_create_rccl: {L.clrrt_xchg_last_error().decode()}")
        self.h = h
        self.cap = int(cap_records)
        if L.clrrt_xchg_attach(h, planner.h) != 0:
            msg = L.clrrt_xchg_last_error().decode()
            self.close()
            raise ClrrtError(f"clrrt_xchg_attach: {msg}")
        self._planner = planner

    def records_ptr(self):
        return self.L.clrrt_xchg_records(self.h)

    def stats(self):
        """exchanges, collectives, second gathers, closing exchanges, rows sent, rows received, the row bound."""
        import ctypes as C
        out = (C.c_int64 * 8)()
        self.L.clrrt_xchg_stats(self.h, out)
        keys = ("exchanges", "collectives", "second_gathers", "closing", "rows_sent", "rows_received", "bound")
        return dict(zip(keys, (int(v) for v in out)))

    def path_rows(self, planner):
        """Complete the committed path's rows across the ranks on the device (clrrt_xchg_path_rows): collective,
        after planner.path_commit on every rank and before path_transform.  Returns the rows this rank took from
        other ranks.  (fetch_path_rows is the same through torch.distributed and the host.)"""
        import ctypes as C
        from . import ClrrtError
        moved = C.c_int64(0)
        rc = self.L.clrrt_xchg_path_rows(self.h, planner.h, C.byref(moved))
        if rc != 0:
            raise ClrrtError(f"clrrt_xchg_path_rows -> {rc}: {self.L.clrrt_xchg_last_error().decode()}")
        return int(moved.value)

    def path_stats(self):
        """completions, collectives, rows gathered, rows taken (clrrt_xchg_path_stats)."""
        import ctypes as C
        out = (C.c_int64 * 4)()
        self.L.clrrt_xchg_path_stats(self.h, out)
        return dict(zip(("completions", "collectives", "rows_gathered", "rows_taken"), (int(v) for v in out)))

    rounds = property(lambda self: self.stats()["exchanges"])
    collectives = property(lambda self: self.stats()["collectives"])
    second_gathers = property(lambda self: self.stats()["second_gathers"])
    closing = property(lambda self: self.stats()["closing"])

    def close(self):
        """Detach from the planner (sharding off) and free the communicator and the buffers."""
        if getattr(self, "h", None):
            pl = getattr(self, "_planner", None)
            if pl is not None and pl.h:
                pl.set_shards(0, 1)
            self.L.clrrt_xchg_destroy(self.h)
            self.h = None


def exchange_capacity(max_batch, defer_steps=0, sim_dt=0.04):
    """Records one rank may commit in a round: 2 per sample of its slice and of its deferred samples (at
    most the ring's R - 1 earlier rounds: R = ceil(2 n_steps / T) + 2, clrrt_capi.hip ensure_defer)."""
    import math
    n_steps = 0
    while n_steps < 20.0 / sim_dt:
        n_steps += 1
    R = (2 * n_steps + defer_steps - 1) // defer_steps + 2 if defer_steps > 0 else 1
    return 2 * max_batch * R


def goal_sum(records):
    """Appended nodes with goalReached set (feasible paths) among the records, as a device tensor (no
    host sync: accumulate per query, read once)."""
    if records.shape[0] == 0:
        return torch.zeros((), dtype=torch.int64, device=records.device)
    return records[:, GOAL_OFFSET:GOAL_OFFSET + 4].contiguous().view(torch.int32).sum(dtype=torch.int64)


def goal_count(records):
    return int(goal_sum(records).item())


def shard(n_total, world, rank):
    """Contiguous slice [first, first + count) of a round's samples handled by `rank` (the engine's
    shard_slice, clrrt_capi.hip)."""
    first = n_total * rank // world
    return first, n_total * (rank + 1) // world - first


def node_range(n_nodes, world, rank):
    """Contiguous node-id range [first, first + count) = [n r / W, n (r + 1) / W) of the tree that `rank` searches in
    a tree-partitioned round (integer arithmetic, as in `shard`); the ranges of all ranks tile [0, n_nodes)."""
    first = n_nodes * rank // world
    return first, n_nodes * (rank + 1) // world - first


class PartitionedSearch:
    """Tree-partitioned nearest-node search of a round (include/clrrt.h): instead of searching the
    whole replicated tree for its slice of the samples, every rank searches ALL G samples over its `node_range` of
    the nodes (clrrt_nn_range), one all-gather moves the ranks' lists (10 ids + 10 keys + a count per sample: 84 G
    bytes per rank), every rank merges them in (key, id) order (clrrt_nn_merge) -- exactly the lists a search of the
    whole tree returns -- and runs its `shard` slice of the round from its rows of the merged lists
    (clrrt_round_eval_lists).  The caller then exchanges and commits the records as after clrrt_round_eval
    (RoundExchange.exchange + Planner.round_commit).  gloo stages the gather through the host, as RoundExchange does.

    The lists stay on the device; the planner's stream must be torch's current stream (Planner.set_stream) or the
    caller must order the two, as for RoundExchange."""

    K = 10
    ROW = 4 * (2 * K + 1)  # bytes per sample: ids, keys, count

    def __init__(self, planner, G, device, group=None):
        if planner.max_batch < G:
            raise ValueError(f"PartitionedSearch: the planner's max_batch ({planner.max_batch}) must be >= the round's "
                             f"{G} samples (every rank searches all of them over its node range)")
        self.pl = planner
        self.G = int(G)
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.dev = torch.device(device)
        self.host = dist.get_backend(group) == "gloo" and self.dev.type != "cpu"
        K = self.K
        # this rank's lists in one buffer (one collective): G x 10 ids | G x 10 key bits | G counts, as int32 words
        self.mine = torch.zeros(self.G * (2 * K + 1), dtype=torch.int32, device=self.dev)
        # the gathered lists in clrrt_nn_merge's layout [part][sample][10] / [part][sample], and the merged lists
        self.ids = torch.zeros((self.world, self.G, K), dtype=torch.int32, device=self.dev)
        self.keys = torch.zeros((self.world, self.G, K), dtype=torch.float32, device=self.dev)
        self.counts = torch.zeros((self.world, self.G), dtype=torch.int32, device=self.dev)
        self.m_ids = torch.zeros((self.G, K), dtype=torch.int32, device=self.dev)
        self.m_keys = torch.zeros((self.G, K), dtype=torch.float32, device=self.dev)
        self.m_counts = torch.zeros(self.G, dtype=torch.int32, device=self.dev)
        self.collectives = 0
        self.bytes_gathered = 0

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.current_stream(self.dev).synchronize()

    def lists(self, samples_all):
        """Steps 1-3: the merged lists of all G samples (device tensors ids (G, 10), keys (G, 10), counts (G,))."""
        G, K = self.G, self.K
        if len(samples_all) != G:
            raise ValueError(f"PartitionedSearch: {len(samples_all)} samples, built for {G}")
        first, count = node_range(self.pl.size()[0], self.world, self.rank)
        base = self.mine.data_ptr()
        self.pl.nn_range(samples_all, first, count, out=(base, base + 4 * G * K, base + 8 * G * K))
        src = self.mine.cpu() if self.host else self.mine
        parts = [torch.empty_like(src) for _ in range(self.world)]
        dist.all_gather(parts, src, group=self.group)
        self.collectives += 1
        self.bytes_gathered += self.world * G * self.ROW
        for r, q in enumerate(parts):
            q = q.to(self.dev)
            self.ids[r].copy_(q[:G * K].view(G, K))
            self.keys[r].copy_(q[G * K:2 * G * K].view(torch.float32).view(G, K))
            self.counts[r].copy_(q[2 * G * K:])
        self._sync()  # the engine reads the gathered lists on its own stream
        self.pl.nn_merge(self.ids.data_ptr(), self.keys.data_ptr(), self.counts.data_ptr(), n=G, parts=self.world,
                         out=(self.m_ids.data_ptr(), self.m_keys.data_ptr(), self.m_counts.data_ptr()))
        return self.m_ids, self.m_keys, self.m_counts

    def round_eval(self, samples_all, records_ptr):
        """One round's evaluate half: searches, gathers and merges the lists of `samples_all` (abi.Sample array of G
        samples, the same on every rank), then evaluates this rank's `shard` slice from its rows of the merged lists,
        writing the accepted-node records to records_ptr (e.g. RoundExchange.records_ptr()).  Returns n_local."""
        from . import abi
        K = self.K
        self.lists(samples_all)
        first, count = shard(self.G, self.world, self.rank)
        mine = (abi.Sample * count).from_buffer_copy(bytes(samples_all)[first * 24:(first + count) * 24])
        return self.pl.round_eval_lists(mine, self.m_ids.data_ptr() + 4 * K * first,
                                        self.m_keys.data_ptr() + 4 * K * first, self.m_counts.data_ptr() + 4 * first,
                                        records_ptr)


def fetch_path_rows(planner, rank, group=None):
    """Complete the committed path's trajectories across ranks (config 5 with N > 1).

    clrrt_path_commit copies the rows of nodes this rank owns and zero-fills the others; the path
    (a few nodes, a few thousand rows) is all-gathered and every node takes its rows from its owner,
    so every rank ends up with the same committed path.  Returns the number of rows moved."""
    import numpy as np
    nodes, rows = planner.path_download()
    if len(nodes) == 0:
        return 0
    world = dist.get_world_size(group)
    cdev = torch.device("cpu") if dist.get_backend(group) == "gloo" else torch.device("cuda", torch.cuda.current_device())
    t = torch.from_numpy(np.ascontiguousarray(rows)).to(cdev)
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t, group=group)
    parts = [p.cpu().numpy() for p in parts]
    fixed = rows.copy()
    moved = 0
    for nd in nodes:
        if nd.owner != rank:
            a, b = nd.row_offset, nd.row_offset + nd.nrows
            fixed[a:b] = parts[nd.owner][a:b]
            moved += nd.nrows
    if moved:
        planner.path_load(nodes, fixed)
    return moved
