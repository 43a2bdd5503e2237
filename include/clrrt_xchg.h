/*
 * clrrt_xchg.h — C-ABI of libclrrt_xchg, the native exchange of libclrrt's sharded expansion.
 *
 * clrrt_set_shards (clrrt.h) takes a hook that all-gathers a round's accepted-node records across the ranks.  This
 * library is that hook, in native code, behind the hook's unchanged signature: a C or C++ host links -lclrrt_xchg
 * -lclrrt and runs clrrt_expand on more than one GPU without writing a collective (and without Python).  libclrrt
 * itself does not depend on it, nor on RCCL.
 *
 * Protocol (clrrt.dist.RoundExchange's).  An exchange object owns the send buffer -- a header row and
 * cap_records rows of 160 bytes (clrrt_node); the engine writes the round's records from row 1 on, which is the
 * dev_local of clrrt_set_shards -- the receive buffers, the concatenation buffer, a pinned summary and the adaptive
 * row bound.  Per exchange the header (n_local, elapsed_ms, aux_local, bbox_local[4]) goes to row 0 and ONE
 * all-gather moves header + the first `bound` rows of every rank; a device kernel (k_xchg_concat) reads the W headers,
 * copies every rank's rows to their place in the contiguous dev_all and writes the summary (counts, n_all, the largest
 * elapsed_ms, the aux sum, the union of the bounds), whose read is the exchange's one host wait.  Only when some
 * rank's count exceeds `bound` a second gather moves the excess rows.  Then bound = max(bound, 1.25 max count + 64),
 * capped at cap_records.  Everything is queued on io->stream (the engine's), so the collective is ordered after the
 * engine's writes and the engine's reads after the collective without host synchronisation.
 *
 * Two transports behind the same hook:
 *   RCCL        one process per GPU; ncclAllGather on io->stream.  The host distributes the unique id.
 *               A closing exchange (io->flags bit 0) moves the round's message size and copies no rows: a rank that
 *               fails leaves its rounds early and closes while its peers are in a round's exchange, and the two must
 *               be the same collective.
 *   in-process  one process, one host thread and one clrrt_ctx per rank, on one device or several (a ROS-free
 *               planner process with N GPUs; also the way to run W > 1 natively on one GPU, where RCCL refuses two
 *               ranks on one device).  Each rank records an event on its stream, the ranks meet at a host rendezvous,
 *               every stream waits for its peers' events and pulls their rows (hipMemcpyAsync / hipMemcpyPeerAsync);
 *               a second rendezvous after the pulls are queued lets the owner's stream wait for the pullers before
 *               the engine's next round overwrites the send buffer.  A closing exchange pulls headers only.  Every
 *               rendezvous wait has the group's deadline: a rank whose peer never arrives returns -1 from the hook
 *               (clrrt_expand then returns CLRRT_EHIP) within timeout_ms.
 *
 * All entry points return an int status: 0 ok, CLRRT_EINVAL (-1), CLRRT_EHIP (-2: a HIP or RCCL call failed, or the
 * rendezvous timed out), CLRRT_ECAPACITY (-3), CLRRT_ESTATE (-4: the ranks' committed paths differ); clrrt_xchg_last_error gives the message of the calling thread's last
 * failure.  An exchange object belongs to one host thread at a time (its rank's), like a clrrt_ctx.
 */
#ifndef CLRRT_XCHG_H
#define CLRRT_XCHG_H

#include <stdint.h>

#include "clrrt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CLRRT_XCHG_MAX_WORLD 64
#define CLRRT_XCHG_UID_BYTES 128

typedef struct clrrt_xchg clrrt_xchg;
typedef struct clrrt_xchg_group clrrt_xchg_group;

/* Message of the calling thread's last failed call ("" when none). */
const char* clrrt_xchg_last_error(void);

/* ---- RCCL transport: one process per GPU ---- */
/* ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to every rank (a file, a socket, MPI, a process group). */
int clrrt_xchg_unique_id(void* out /* [CLRRT_XCHG_UID_BYTES] */);
/* ncclCommInitRank on `device` + the buffers.  1 <= world <= 64, 0 <= rank < world, cap_records >= 1 (the cap_local of
 * clrrt_set_shards: clrrt.dist.exchange_capacity), first_bound >= 1 (rows of the first all-gather; this rank's slice
 * size + 64 covers the first rounds without a second gather; clamped to cap_records; the same on every rank). */
int clrrt_xchg_create_rccl(const void* uid, int32_t rank, int32_t world, int32_t device, int32_t cap_records,
                           int32_t first_bound, clrrt_xchg** out);

/* ---- in-process transport: one thread and one clrrt_ctx per rank ---- */
/* The ranks' meeting point.  timeout_ms > 0: the deadline of every rendezvous wait. */
int clrrt_xchg_group_create(int32_t world, int32_t timeout_ms, clrrt_xchg_group** out);
/* After every exchange object made from it was destroyed. */
void clrrt_xchg_group_destroy(clrrt_xchg_group* g);
/* Rank `rank` of the group on `device` (ranks may share a device).  Each rank is created once; all ranks must exist
 * before the first exchange (a hook that finds a peer missing waits for it until the deadline). */
int clrrt_xchg_create_local(clrrt_xchg_group* g, int32_t rank, int32_t device, int32_t cap_records,
                            int32_t first_bound, clrrt_xchg** out);

/* ---- common ---- */
/* The hook: a clrrt_exchange_fn whose `user` is the exchange object (contract: clrrt.h, clrrt_exchange_io). */
int32_t clrrt_xchg_hook(void* user, clrrt_exchange_io* io);
/* clrrt_set_shards(ctx, rank, world, clrrt_xchg_records(x), cap_records, clrrt_xchg_hook, x).  With world 1 the
 * context's option "shard_hook_world1" must be 1 for the hook to be kept. */
int clrrt_xchg_attach(clrrt_xchg* x, clrrt_ctx* ctx);
/* Device address of the send rows (row 1 of the send buffer); NULL for a null object. */
void* clrrt_xchg_records(clrrt_xchg* x);
/* out[0] exchanges, out[1] collectives (all-gathers; in-process: pull rounds), out[2] second gathers, out[3] closing
 * exchanges, out[4] record rows sent (this rank's counts), out[5] record rows received (all ranks' counts of the
 * non-closing exchanges), out[6] the current row bound, out[7] 0. */
int clrrt_xchg_stats(clrrt_xchg* x, int64_t out[8]);
void clrrt_xchg_destroy(clrrt_xchg* x);

/* ---- the committed path's rows across ranks (a sharded planMotion: 5 Hz replanning from the committed path) ----
 * In a sharded expansion a node's trajectory rows stay on the rank that grew it (clrrt_node::owner), so
 * clrrt_path_commit leaves the rows of foreign nodes zero-filled.  Every rank commits the same node ids (the headers
 * are replicated), so the paths have the same n and the same path-local row layout; but the ranks do NOT agree on
 * `owner` for every node: a node kept by clrrt_tree_init_from_path is stamped with the local rank on every rank (each
 * holds its own copy of those rows), only a node grown in a sharded round has one owner for all.  So every rank offers
 * its whole path row buffer (R rows, zeros where foreign) and the receiver picks per node by ITS OWN view of owner:
 *   1. agreement: the host reads the n headers once -- the completion's host wait -- and hashes their first 148
 *      bytes; (n, R, hash) of every rank is gathered and compared on the host (in-process through the rendezvous;
 *      RCCL by a 32-byte all-gather, whose read is a second wait there).  If a rank differs, every rank returns
 *      CLRRT_ESTATE (the message names the first rank that differs from rank 0) and no row collective is started, so
 *      a collective with unequal counts cannot happen.  n = 0 everywhere: ok, 0 rows.
 *   2. rows: RCCL -- one ncclAllGather of R x 80 bytes on the engine's stream; in-process -- the ranks publish their
 *      row pointer and an event, meet, and each pulls the buffers of the ranks that own a node it needs (no others);
 *      a second meeting keeps an owner from changing its path before the pullers' copies are done.
 *   3. selection: k_xchg_path_select copies, for every node whose owner is another rank, that rank's rows into the
 *      context's path rows (clrrt_path_device) as raw bits (the sign of zero and NaN payloads survive).
 * All of it is queued on the context's stream (the one the attached context's last exchange ran on).
 * A rank that fails between its expansion and the completion leaves its peers in the completion: the in-process
 * transport bounds that wait by the group's deadline (CLRRT_EHIP); RCCL cannot bound it (the collective waits for the
 * missing rank), so an RCCL host that abandons a query must tear its communicator down.
 *
 * Collective over the exchange's ranks, after clrrt_path_commit on every rank and before clrrt_path_transform: every
 * path node whose rows this rank does not own takes them from its owner.  user = the clrrt_xchg object (the
 * signature is the adapter's path-completer hook).  *rows_moved: rows this rank received into its path. */
int32_t clrrt_xchg_path_rows(void* user, clrrt_ctx* ctx, int64_t* rows_moved);
int clrrt_xchg_path_stats(clrrt_xchg* x, int64_t out[4]); /* completions, collectives, rows gathered, rows taken */

/* Test hook: k_xchg_concat on `device` over patterned parts.  W parts of (bound + 1) rows (row 0 a header with
 * counts[r], elapsed[r], aux[r], bbox[4 r .. 4 r + 4)) and, with excess_rows > 0, W excess parts of excess_rows rows
 * (rows bound .. of each rank).  Row j of rank r is filled with the bytes (uint8)(r * 131 + j * 7 + b * 3 + 1) for
 * byte b = 0 .. 159.  Writes the sum(counts) concatenated rows to out_rows (out_cap rows of 160 bytes) and the
 * summary to summary[8 + W]: n_all, the largest count, the largest elapsed (double bits), the aux sum, the bounds'
 * union x0, y0, x1, y1 (double bits), then the W counts.  CLRRT_EINVAL for W outside [1, 64], bound < 1, a negative
 * count, a count above bound + excess_rows, or out_cap < sum(counts). */
int clrrt_xchg_selftest_concat(int32_t device, int32_t W, int32_t bound, const int32_t* counts, const double* elapsed,
                               const int64_t* aux, const double* bbox, int32_t excess_rows, void* out_rows,
                               int64_t out_cap, int64_t* summary);

/* Test hook: k_xchg_path_select on `device` as rank `self` of W over a path of n nodes (owners[i] in [0, W),
 * nrows[i] >= 1; row offsets are the prefix sums of nrows, R their total) and W patterned parts of R rows.  Entry
 * (row j, column c) of rank r's part is the raw 64-bit pattern, with b = (r + 1) << 44 | j << 8 | c and k = (j + c) % 5:
 *   k = 0: b (a subnormal)         k = 1: 0x7FF8000000000000 | b (a quiet NaN with payload b)
 *   k = 2: 0xFFF0000000000000 | b (a negative signalling NaN, payload b)
 *   k = 3: 0x8000000000000000 (-0.0)         k = 4: 0x4000000000000000 | b (a finite number)
 * The rank's own rows are pre-filled with its own pattern (r = self).  Writes the R rows after the selection to
 * out_rows (R x 10 doubles) and the rows taken from other ranks to *out_moved.  CLRRT_EINVAL for W outside [1, 64],
 * self outside [0, W), n < 0, an owner outside [0, W) or nrows[i] < 1. */
int clrrt_xchg_selftest_path_select(int32_t device, int32_t W, int32_t self, int32_t n, const int32_t* owners,
                                    const int32_t* nrows, void* out_rows, int64_t* out_moved);

#ifdef __cplusplus
}
#endif

#endif /* CLRRT_XCHG_H */
