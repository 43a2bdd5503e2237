// libclrrt_xchg.so — the native exchange of the sharded expansion (include/clrrt_xchg.h): RoundExchange's
// count-prefixed all-gather (clrrt/dist.py) behind clrrt_set_shards' hook, over RCCL (one process per GPU) or over an
// in-process rendezvous with peer copies (one thread per rank), and the kernel both share, k_xchg_concat; and the
// completion of the committed path's rows across the ranks (clrrt_xchg_path_rows, k_xchg_path_select).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clrrt_xchg.h"
#include "clrrt_devmem_hip.hpp"
#include "clrrt_rendezvous.hpp"

namespace {

constexpr int ROW = 160;            // sizeof(clrrt_node): one record row
constexpr int ROW_V = ROW / 16;     // 16-byte vectors per row
constexpr int MAXW = CLRRT_XCHG_MAX_WORLD;
static_assert(sizeof(clrrt_node) == ROW, "record rows are clrrt_node");

// row 0 of every send buffer (RoundExchange.HDR: 56 bytes)
struct Header {
  int64_t n;
  double elapsed;
  int64_t aux;
  double bbox[4];
};
static_assert(sizeof(Header) == 56 && sizeof(Header) <= ROW, "header row");

struct Summary {
  int64_t n_all;
  int64_t max_count;
  double max_elapsed;
  int64_t aux_sum;
  double bbox[4];
  int64_t counts[MAXW];
};

struct ConcatArgs {
  const uint4* parts;   // [W][part_stride] rows, row 0 of a part its header, then the first `bound` record rows
  const uint4* excess;  // [W][ex_stride] rows: record rows bound .. of every rank (second gather), or null
  uint4* out;           // the records of all ranks, contiguous in rank order
  Summary* summary;
  int64_t part_stride, ex_stride;  // rows
  int64_t ex_rows;                 // valid rows of an excess part
  int64_t cap_rows;                // record rows a rank can send
  int64_t out_cap;                 // rows
  int W, bound;
  int copy_first, copy_excess;
};

// One launch per round on the engine's stream.  Every block reads the W headers (W <= 64: one wave's worth) and forms
// the prefix of the counts in LDS; the blocks then copy part r's rows to rows [prefix_r, prefix_r + count_r) of `out`,
// rank by rank, grid-stride over 16-byte vectors: consecutive lanes move consecutive vectors of the (contiguous) rows,
// so loads and stores are coalesced 1 KiB wave accesses.  Rows below `bound` come from the first gather's parts
// (copy_first), rows from `bound` on from the excess parts (copy_excess; a second launch after the rare second
// gather, or the same launch in the selftest): the prefix is that of the whole counts in either launch, so the two
// fill disjoint rows.  Counts are clamped to a rank's capacity, the total to `out`'s and every copy to the rows its
// source holds, so a corrupt header cannot send an access out of bounds (the host rejects such a summary).  Thread 0
// of block 0 writes the summary.
__global__ __launch_bounds__(256) void k_xchg_concat(ConcatArgs a) {
  __shared__ int64_t s_cnt[MAXW];
  __shared__ int64_t s_off[MAXW + 1];
  const int t = threadIdx.x;
  if (t < a.W) s_cnt[t] = reinterpret_cast<const Header*>(a.parts + (int64_t)t * a.part_stride * ROW_V)->n;
  __syncthreads();
  if (t == 0) {
    int64_t off = 0;
    for (int r = 0; r < a.W; r++) {
      s_off[r] = off;
      int64_t c = s_cnt[r];
      c = c < 0 ? 0 : (c > a.cap_rows ? a.cap_rows : c);
      if (off + c > a.out_cap) c = a.out_cap - off;
      off += c;
    }
    s_off[a.W] = off;
  }
  __syncthreads();
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + t;
  const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int r = 0; r < a.W; r++) {
    const int64_t cnt = s_off[r + 1] - s_off[r];
    const int64_t first = cnt < a.bound ? cnt : a.bound;
    uint4* dst = a.out + s_off[r] * ROW_V;
    if (a.copy_first) {
      const uint4* src = a.parts + ((int64_t)r * a.part_stride + 1) * ROW_V;
      for (int64_t v = gtid; v < first * ROW_V; v += gstride) dst[v] = src[v];
    }
    if (a.copy_excess && a.excess && cnt > first) {
      const uint4* src = a.excess + (int64_t)r * a.ex_stride * ROW_V;
      uint4* dx = dst + first * ROW_V;
      const int64_t more = cnt - first < a.ex_rows ? cnt - first : a.ex_rows;
      for (int64_t v = gtid; v < more * ROW_V; v += gstride) dx[v] = src[v];
    }
  }
  if (blockIdx.x == 0 && t == 0) {
    Summary s;
    s.n_all = 0;
    s.max_count = 0;
    s.max_elapsed = -HUGE_VAL;
    s.aux_sum = 0;
    s.bbox[0] = s.bbox[1] = HUGE_VAL;
    s.bbox[2] = s.bbox[3] = -HUGE_VAL;
    Summary* o = a.summary;
    for (int r = 0; r < a.W; r++) {
      const Header h = *reinterpret_cast<const Header*>(a.parts + (int64_t)r * a.part_stride * ROW_V);
      o->counts[r] = h.n;
      s.n_all += h.n;
      s.max_count = h.n > s.max_count ? h.n : s.max_count;
      s.max_elapsed = h.elapsed > s.max_elapsed ? h.elapsed : s.max_elapsed;
      s.aux_sum += h.aux;
      s.bbox[0] = h.bbox[0] < s.bbox[0] ? h.bbox[0] : s.bbox[0];
      s.bbox[1] = h.bbox[1] < s.bbox[1] ? h.bbox[1] : s.bbox[1];
      s.bbox[2] = h.bbox[2] > s.bbox[2] ? h.bbox[2] : s.bbox[2];
      s.bbox[3] = h.bbox[3] > s.bbox[3] ? h.bbox[3] : s.bbox[3];
    }
    for (int r = a.W; r < MAXW; r++) o->counts[r] = 0;
    o->n_all = s.n_all;
    o->max_count = s.max_count;
    o->max_elapsed = s.max_elapsed;
    o->aux_sum = s.aux_sum;
    for (int q = 0; q < 4; q++) o->bbox[q] = s.bbox[q];
  }
}

hipError_t launch_concat(hipStream_t st, const ConcatArgs& a, int64_t rows_per_part) {
  // one vector per lane where the round is small; at most 256 blocks (one per CU) striding over a large one
  const int64_t vec = std::max<int64_t>(1, rows_per_part * ROW_V);
  const int blocks = (int)std::min<int64_t>(256, (vec + 255) / 256);
  hipLaunchKernelGGL(k_xchg_concat, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---- the committed path's rows (clrrt_xchg_path_rows)
constexpr int PROW_V = 5;      // 16-byte vectors per trajectory row (10 doubles)
constexpr int PROW = 80;       // bytes per trajectory row
constexpr int PHDR = 148;      // clrrt_node bytes before owner / row_offset: what the ranks must agree on
constexpr int PSEL_CHUNK = 256;  // path nodes a block holds in LDS at a time (one per thread)

// what the ranks compare before any row moves
struct PathHdr {
  int64_t n, rows;
  uint64_t hash;  // FNV-1a over the n headers' first PHDR bytes
  int64_t pad;
};
static_assert(sizeof(PathHdr) == 32, "agreement record");

struct PathSelectArgs {
  const uint4* parts;        // [W][rows] trajectory rows: every rank's whole path row buffer (zeros where foreign)
  uint4* dst;                // this rank's path rows
  const clrrt_node* nodes;   // this rank's n path headers (path-local row_offset, its own view of owner)
  int64_t rows;              // R
  int n, W, self;
};

// One launch per completion on the engine's stream.  The path's nodes are taken PSEL_CHUNK at a time: thread t loads
// node c0 + t's row range [start, end) and owner into LDS (clamped to [0, R] and start <= end, so nothing below can
// index outside the buffers whatever the header holds), then the grid strides over the 16-byte vectors of the
// chunk's rows -- 5 per 80-byte row, consecutive lanes consecutive vectors, so a wave's access is one contiguous
// 1 KiB although node borders fall inside it -- and each vector finds its node by a binary search over the chunk's
// starts (the last node whose start is <= the vector's row).  A vector of a node owned by another rank is copied
// from that rank's part, as raw bits; a node this rank owns (or whose owner is no rank) is left alone.
__global__ __launch_bounds__(256) void k_xchg_path_select(PathSelectArgs a) {
  __shared__ int64_t s_start[PSEL_CHUNK];
  __shared__ int64_t s_end[PSEL_CHUNK];
  __shared__ int s_own[PSEL_CHUNK];
  const int t = threadIdx.x;
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + t;
  const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int c0 = 0; c0 < a.n; c0 += PSEL_CHUNK) {
    const int cnt = a.n - c0 < PSEL_CHUNK ? a.n - c0 : PSEL_CHUNK;
    __syncthreads();  // the last chunk's searches are done
    if (t < cnt) {
      const clrrt_node* nd = a.nodes + c0 + t;
      int64_t s = nd->row_offset, e = nd->row_offset + (int64_t)nd->nrows;
      s = s < 0 ? 0 : (s > a.rows ? a.rows : s);
      e = e < s ? s : (e > a.rows ? a.rows : e);
      s_start[t] = s;
      s_end[t] = e;
      s_own[t] = nd->owner;
    }
    __syncthreads();
    const int64_t lo = s_start[0], hi = s_end[cnt - 1];
    for (int64_t v = lo * PROW_V + gtid; v < hi * PROW_V; v += gstride) {
      const int64_t row = v / PROW_V;
      int i = 0, j = cnt - 1;  // the last node of the chunk whose start is <= row
      while (i < j) {
        const int m = (i + j + 1) >> 1;
        if (s_start[m] <= row) i = m;
        else j = m - 1;
      }
      const int own = s_own[i];
      if (row >= s_start[i] && row < s_end[i] && own != a.self && own >= 0 && own < a.W)
        a.dst[v] = a.parts[(int64_t)own * a.rows * PROW_V + v];
    }
  }
}

hipError_t launch_path_select(hipStream_t st, const PathSelectArgs& a) {
  const int64_t vec = std::max<int64_t>(1, a.rows * PROW_V);
  const int blocks = (int)std::min<int64_t>(256, (vec + 255) / 256);
  hipLaunchKernelGGL(k_xchg_path_select, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

uint64_t path_hash(const clrrt_node* h, int n) {
  uint64_t x = 0xcbf29ce484222325ull;
  for (int i = 0; i < n; i++) {
    const unsigned char* b = (const unsigned char*)&h[i];
    for (int k = 0; k < PHDR; k++) x = (x ^ b[k]) * 0x100000001b3ull;
  }
  return x;
}

thread_local std::string t_err;
int fail(int code, const std::string& msg) {
  t_err = msg;
  return code;
}
#define XHIP(expr)                                                                                   \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return fail(CLRRT_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
const char* nccl_name(ncclResult_t r) {
  switch (r) {
    case ncclUnhandledCudaError: return "ncclUnhandledCudaError";
    case ncclSystemError: return "ncclSystemError";
    case ncclInternalError: return "ncclInternalError";
    case ncclInvalidArgument: return "ncclInvalidArgument";
    case ncclInvalidUsage: return "ncclInvalidUsage";
    case ncclRemoteError: return "ncclRemoteError";
    default: return "ncclError";
  }
}
#define XNCCL(expr)                                                                                          \
  do {                                                                                                       \
    ncclResult_t e_ = (expr);                                                                                \
    if (e_ != ncclSuccess)                                                                                   \
      return fail(CLRRT_EHIP, std::string(#expr) + ": " + ncclGetErrorString(e_) + " (" + nccl_name(e_) + ")"); \
  } while (0)

}  // namespace

// one rank's published state in an in-process group (written at creation / before a meeting, read after it)
struct LocalSlot {
  clrrt_xchg* x = nullptr;
  int closing = 0;  // this exchange is the rank's closing one
  // the path completion: this rank's agreement record and its path row buffer (R rows)
  PathHdr path{};
  const char* path_rows = nullptr;
};

struct clrrt_xchg_group {
  clrrt_xchg_detail::Rendezvous rv;
  std::mutex m;  // creation of the ranks
  LocalSlot slot[MAXW];
  clrrt_xchg_group(int world, int timeout_ms) : rv(world, timeout_ms) {}
};

struct clrrt_xchg {
  int rank = 0, world = 1, device = 0;
  clrrt::DevMem<HipMem> mem;  // every device and pinned buffer below is its (freed by clrrt_xchg_destroy)
  int64_t cap = 0;    // record rows of the send buffer (besides the header row)
  int64_t bound = 0;  // rows of the first gather
  char* send = nullptr;     // [cap + 1] rows
  char* recv = nullptr;     // [world][cap + 1] rows (a gather of bound + 1 rows packs them [world][bound + 1])
  char* recv_ex = nullptr;  // [world][cap] rows, made at the first second gather
  char* out = nullptr;      // [world * cap] rows
  Summary* d_sum = nullptr;
  Summary* h_sum = nullptr;  // pinned
  Header* h_hdr = nullptr;   // pinned staging of the header row
  hipEvent_t ev_sum = nullptr;
  // RCCL
  ncclComm_t comm = nullptr;
  // in-process
  clrrt_xchg_group* group = nullptr;
  hipEvent_t ev_sent = nullptr;    // this rank's rows are written (peers wait for it before pulling)
  hipEvent_t ev_pulled = nullptr;  // this rank's pulls are done (the owners wait for it before going on)
  int64_t st[8] = {};
  // the path completion (clrrt_xchg_path_rows)
  clrrt_ctx* ctx = nullptr;        // the attached context
  hipStream_t stream = nullptr;    // its stream, as the last exchange saw it
  bool have_stream = false;
  clrrt_node* h_nodes = nullptr;   // pinned: this rank's path headers
  int h_nodes_cap = 0;
  char* p_recv = nullptr;          // [world][R] trajectory rows, grown on demand
  int64_t p_recv_rows = 0;         // rows it holds
  PathHdr* d_phdr = nullptr;       // RCCL: [1 + world] agreement records (this rank's, then the gathered ones)
  PathHdr* h_phdr = nullptr;       // pinned [1 + world]
  int64_t pst[4] = {};
};

namespace {

int alloc_common(clrrt_xchg* x) {
  const size_t part = (size_t)(x->cap + 1) * ROW;
  XHIP(hipSetDevice(x->device));
  XHIP(x->mem.renew(&x->send, part));
  XHIP(hipMemset(x->send, 0, part));
  XHIP(x->mem.renew(&x->recv, part * x->world));
  XHIP(x->mem.renew(&x->out, (size_t)x->cap * ROW * x->world));
  XHIP(x->mem.renew(&x->d_sum, 1));
  XHIP(x->mem.renew_host(&x->h_sum, 1));
  XHIP(x->mem.renew_host(&x->h_hdr, 1));
  XHIP(hipEventCreateWithFlags(&x->ev_sum, hipEventDisableTiming));
  XHIP(x->mem.renew(&x->d_phdr, 1 + x->world));
  XHIP(x->mem.renew_host(&x->h_phdr, 1 + x->world));
  return CLRRT_OK;
}

int check_create(int32_t rank, int32_t world, int32_t device, int32_t cap_records, int32_t first_bound, void* out) {
  if (!out || world < 1 || world > MAXW || rank < 0 || rank >= world || device < 0 || cap_records < 1 ||
      first_bound < 1)
    return fail(CLRRT_EINVAL, "clrrt_xchg: bad argument (1 <= world <= 64, 0 <= rank < world, cap_records >= 1, "
                              "first_bound >= 1, a non-null result pointer)");
  return CLRRT_OK;
}

// Rows of every part in this exchange's first gather (header included), and the stride of the gathered parts.
struct Plan {
  int64_t rows, stride;
};

// The concat launch(es), the summary's read and the second gather around `gather(first_row, rows, dst, stride)`,
// which moves rows [first_row, first_row + rows) of every rank's send buffer to dst[rank * stride rows].
template <class Gather>
int run_exchange(clrrt_xchg* x, clrrt_exchange_io* io, hipStream_t st, bool copy_rows, bool gather_excess,
                 const Plan& p, Gather&& gather) {
  int rc = gather(0, p.rows, x->recv, p.stride);
  if (rc != CLRRT_OK) return rc;
  x->st[1]++;
  ConcatArgs a{};
  a.parts = (const uint4*)x->recv;
  a.out = (uint4*)x->out;
  a.summary = x->d_sum;
  a.part_stride = p.stride;
  a.out_cap = x->cap * x->world;
  a.cap_rows = x->cap;
  a.W = x->world;
  a.bound = (int)x->bound;
  a.copy_first = copy_rows ? 1 : 0;
  XHIP(launch_concat(st, a, copy_rows ? x->bound : 0));
  XHIP(hipMemcpyAsync(x->h_sum, x->d_sum, sizeof(Summary), hipMemcpyDeviceToHost, st));
  XHIP(hipEventRecord(x->ev_sum, st));
  XHIP(hipEventSynchronize(x->ev_sum));  // the exchange's one host wait
  const Summary& s = *x->h_sum;
  for (int r = 0; r < x->world; r++)
    if (s.counts[r] < 0 || s.counts[r] > x->cap)
      return fail(CLRRT_EHIP, "clrrt_xchg: rank " + std::to_string(r) + " sent a count of " +
                                  std::to_string((long long)s.counts[r]) + " records (capacity " +
                                  std::to_string((long long)x->cap) + "): the ranks' buffers differ or a header is corrupt");
  if (s.n_all > INT32_MAX) return fail(CLRRT_ECAPACITY, "clrrt_xchg: more than 2^31 records in one round");
  if (s.max_count > x->bound && gather_excess) {
    const int64_t ex = s.max_count - x->bound;
    if (!x->recv_ex) XHIP(x->mem.renew(&x->recv_ex, (size_t)x->cap * ROW * x->world));
    if ((rc = gather(1 + x->bound, ex, x->recv_ex, ex)) != CLRRT_OK) return rc;
    x->st[1]++;
    x->st[2]++;
    if (copy_rows) {
      a.excess = (const uint4*)x->recv_ex;
      a.ex_stride = ex;
      a.ex_rows = ex;
      a.copy_first = 0;
      a.copy_excess = 1;
      a.summary = x->d_sum;  // rewritten with the same values
      XHIP(launch_concat(st, a, ex));
    }
  }
  x->bound = std::min<int64_t>(x->cap, std::max<int64_t>(x->bound, (int64_t)(s.max_count * 1.25) + 64));
  x->st[6] = x->bound;
  io->n_all = copy_rows ? (int32_t)s.n_all : 0;
  io->dev_all = io->n_all > 0 ? (void*)x->out : nullptr;
  io->max_elapsed_ms = s.max_elapsed;
  io->aux_sum = s.aux_sum;
  for (int q = 0; q < 4; q++) io->bbox_all[q] = s.bbox[q];
  if (copy_rows) x->st[5] += s.n_all;
  return CLRRT_OK;
}

int hook_rccl(clrrt_xchg* x, clrrt_exchange_io* io, hipStream_t st, bool closing) {
  // a closing exchange is the same collective as a round's (a failed rank closes while its peers are in a round)
  const Plan p{x->bound + 1, x->bound + 1};
  auto gather = [&](int64_t first, int64_t rows, char* dst, int64_t) -> int {
    XNCCL(ncclAllGather(x->send + first * ROW, dst, (size_t)rows * ROW, ncclChar, x->comm, st));
    return CLRRT_OK;
  };
  return run_exchange(x, io, st, !closing, true, p, gather);
}

int hook_local(clrrt_xchg* x, clrrt_exchange_io* io, hipStream_t st, bool closing) {
  clrrt_xchg_group* g = x->group;
  const int W = x->world;
  g->slot[x->rank].closing = closing ? 1 : 0;
  if (hipEventRecord(x->ev_sent, st) != hipSuccess) {
    g->rv.abandon();  // the peers leave their meeting at once
    return fail(CLRRT_EHIP, "clrrt_xchg: hipEventRecord failed");
  }
  if (!g->rv.meet()) return fail(CLRRT_EHIP, "clrrt_xchg: a peer did not reach the exchange within the group's deadline");
  int rc = CLRRT_OK;
  for (int p = 0; p < W && rc == CLRRT_OK; p++) {
    const clrrt_xchg* y = g->slot[p].x;
    if (!y || y->cap != x->cap) rc = fail(CLRRT_EINVAL, "clrrt_xchg: the group's ranks differ in cap_records");
  }
  if (rc == CLRRT_OK) {
    // a closing exchange pulls the headers only (and its peers' rows are of no use to it)
    const Plan p{closing ? 1 : x->bound + 1, x->cap + 1};
    bool waited = false;
    auto gather = [&](int64_t first, int64_t rows, char* dst, int64_t stride) -> int {
      for (int q = 0; q < W; q++) {
        const clrrt_xchg* y = g->slot[q].x;
        if (q != x->rank && !waited) XHIP(hipStreamWaitEvent(st, y->ev_sent, 0));
        const char* src = y->send + first * ROW;
        char* d = dst + (size_t)q * stride * ROW;
        if (y->device == x->device)
          XHIP(hipMemcpyAsync(d, src, (size_t)rows * ROW, hipMemcpyDeviceToDevice, st));
        else
          XHIP(hipMemcpyPeerAsync(d, x->device, src, y->device, (size_t)rows * ROW, st));
      }
      waited = true;
      return CLRRT_OK;
    };
    rc = run_exchange(x, io, st, !closing, !closing, p, gather);
  }
  if (rc == CLRRT_OK && hipEventRecord(x->ev_pulled, st) != hipSuccess)
    rc = fail(CLRRT_EHIP, "clrrt_xchg: hipEventRecord failed");
  if (rc != CLRRT_OK) {
    g->rv.abandon();  // the peers leave their second meeting at once
    return rc;
  }
  // the owners' streams go on (the engine's next round overwrites the send rows) only after every puller's copies
  if (!g->rv.meet()) return fail(CLRRT_EHIP, "clrrt_xchg: a peer left the exchange before its copies were queued");
  for (int q = 0; q < W; q++)
    if (q != x->rank) XHIP(hipStreamWaitEvent(st, g->slot[q].x->ev_pulled, 0));
  return CLRRT_OK;
}

// ---- the path completion
struct PathView {
  clrrt_node* d_nodes = nullptr;
  double* d_rows = nullptr;
  int32_t n = 0;
  int64_t rows = 0;
  int64_t moved = 0;          // rows of the nodes another rank owns
  bool need[MAXW] = {};       // ranks that own a node of the path (other than this rank)
};

int path_grow_recv(clrrt_xchg* x, int64_t rows) {
  if (rows * x->world <= x->p_recv_rows) return CLRRT_OK;
  const int64_t cap = std::max<int64_t>(rows * x->world, 2 * x->p_recv_rows);
  x->p_recv_rows = 0;
  XHIP(x->mem.renew(&x->p_recv, (size_t)cap * PROW));  // (the device free waits for the last completion's kernel)
  x->p_recv_rows = cap;
  return CLRRT_OK;
}

// The first rank whose agreement record differs from rank 0's (-1: none), and the error every rank then returns.
int path_disagreement(const clrrt_xchg* x, const PathHdr* all) {
  for (int r = 1; r < x->world; r++)
    if (all[r].n != all[0].n || all[r].rows != all[0].rows || all[r].hash != all[0].hash) return r;
  return -1;
}
int path_estate(const clrrt_xchg* x, const PathHdr* all, int r) {
  return fail(CLRRT_ESTATE, "clrrt_xchg_path_rows: the committed path of rank " + std::to_string(r) + " (" +
                                std::to_string((long long)all[r].n) + " nodes, " +
                                std::to_string((long long)all[r].rows) + " rows) differs from rank 0's (" +
                                std::to_string((long long)all[0].n) + " nodes, " +
                                std::to_string((long long)all[0].rows) + " rows" +
                                (all[r].n == all[0].n && all[r].rows == all[0].rows ? ", other headers" : "") +
                                "): no rows were moved (seen by rank " + std::to_string(x->rank) + ")");
}

int path_select(clrrt_xchg* x, const PathView& v, hipStream_t st) {
  PathSelectArgs a{};
  a.parts = (const uint4*)x->p_recv;
  a.dst = (uint4*)v.d_rows;
  a.nodes = v.d_nodes;
  a.rows = v.rows;
  a.n = v.n;
  a.W = x->world;
  a.self = x->rank;
  XHIP(launch_path_select(st, a));
  return CLRRT_OK;
}

int path_rccl(clrrt_xchg* x, const PathView& v, const PathHdr& mine, hipStream_t st) {
  // the agreement records travel through the device (RCCL is the only transport between the processes): a second
  // host wait, before which no row collective is queued
  x->h_phdr[0] = mine;
  XHIP(hipMemcpyAsync(x->d_phdr, x->h_phdr, sizeof(PathHdr), hipMemcpyHostToDevice, st));
  XNCCL(ncclAllGather(x->d_phdr, x->d_phdr + 1, sizeof(PathHdr), ncclChar, x->comm, st));
  XHIP(hipMemcpyAsync(x->h_phdr + 1, x->d_phdr + 1, sizeof(PathHdr) * x->world, hipMemcpyDeviceToHost, st));
  XHIP(hipEventRecord(x->ev_sum, st));
  XHIP(hipEventSynchronize(x->ev_sum));
  x->pst[1]++;
  const int bad = path_disagreement(x, x->h_phdr + 1);
  if (bad >= 0) return path_estate(x, x->h_phdr + 1, bad);
  if (v.rows == 0) return CLRRT_OK;
  int rc = path_grow_recv(x, v.rows);
  if (rc != CLRRT_OK) return rc;
  XNCCL(ncclAllGather(v.d_rows, x->p_recv, (size_t)v.rows * PROW, ncclChar, x->comm, st));
  x->pst[1]++;
  x->pst[2] += v.rows * x->world;
  return path_select(x, v, st);
}

int path_local(clrrt_xchg* x, const PathView& v, const PathHdr& mine, hipStream_t st) {
  clrrt_xchg_group* g = x->group;
  const int W = x->world;
  LocalSlot& me = g->slot[x->rank];
  me.path = mine;
  me.path_rows = (const char*)v.d_rows;
  if (hipEventRecord(x->ev_sent, st) != hipSuccess) {
    g->rv.abandon();
    return fail(CLRRT_EHIP, "clrrt_xchg_path_rows: hipEventRecord failed");
  }
  if (!g->rv.meet())
    return fail(CLRRT_EHIP, "clrrt_xchg_path_rows: a peer did not reach the path completion within the group's deadline");
  x->pst[1]++;
  PathHdr all[MAXW];
  for (int q = 0; q < W; q++) all[q] = g->slot[q].path;
  const int bad = path_disagreement(x, all);  // every rank reads the same records: the same verdict everywhere
  int rc = CLRRT_OK;
  if (bad < 0 && v.moved > 0) {
    rc = path_grow_recv(x, v.rows);
    for (int q = 0; q < W && rc == CLRRT_OK; q++) {
      if (!v.need[q]) continue;  // nothing is pulled from a rank that owns no node of the path
      const clrrt_xchg* y = g->slot[q].x;
      auto pull = [&]() -> int {
        if (!y || !g->slot[q].path_rows) return fail(CLRRT_EINVAL, "clrrt_xchg_path_rows: a peer published no path rows");
        XHIP(hipStreamWaitEvent(st, y->ev_sent, 0));
        char* d = x->p_recv + (size_t)q * v.rows * PROW;
        if (y->device == x->device)
          XHIP(hipMemcpyAsync(d, g->slot[q].path_rows, (size_t)v.rows * PROW, hipMemcpyDeviceToDevice, st));
        else
          XHIP(hipMemcpyPeerAsync(d, x->device, g->slot[q].path_rows, y->device, (size_t)v.rows * PROW, st));
        return CLRRT_OK;
      };
      rc = pull();
      if (rc == CLRRT_OK) x->pst[2] += v.rows;
    }
    if (rc == CLRRT_OK) {
      x->pst[1]++;
      rc = path_select(x, v, st);
    }
  }
  if (rc == CLRRT_OK && hipEventRecord(x->ev_pulled, st) != hipSuccess)
    rc = fail(CLRRT_EHIP, "clrrt_xchg_path_rows: hipEventRecord failed");
  if (rc != CLRRT_OK) {
    g->rv.abandon();
    return rc;
  }
  // no owner goes on to change its path (the next query's transform) before every puller's copies are done; the
  // meeting also keeps the published records in place until every rank has read them
  if (!g->rv.meet()) return fail(CLRRT_EHIP, "clrrt_xchg_path_rows: a peer left the path completion before its copies were queued");
  if (bad >= 0) return path_estate(x, all, bad);
  for (int q = 0; q < W; q++)
    if (q != x->rank) XHIP(hipStreamWaitEvent(st, g->slot[q].x->ev_pulled, 0));
  return CLRRT_OK;
}

}  // namespace

extern "C" {

const char* clrrt_xchg_last_error(void) { return t_err.c_str(); }

int32_t clrrt_xchg_path_rows(void* user, clrrt_ctx* ctx, int64_t* rows_moved) {
  clrrt_xchg* x = (clrrt_xchg*)user;
  if (rows_moved) *rows_moved = 0;
  if (!x || !ctx) return fail(CLRRT_EINVAL, "clrrt_xchg_path_rows: null argument");
  if (x->ctx != ctx) return fail(CLRRT_EINVAL, "clrrt_xchg_path_rows: the exchange is not attached to this context");
  if (!x->have_stream)
    return fail(CLRRT_ESTATE, "clrrt_xchg_path_rows: no exchange has run yet (the context's stream is taken from "
                              "the expansion's exchanges)");
  hipStream_t st = x->stream;
  XHIP(hipSetDevice(x->device));
  PathView v;
  void* dn = nullptr;
  if (clrrt_path_device(ctx, &dn, &v.d_rows, &v.n, &v.rows) != CLRRT_OK)
    return fail(CLRRT_EINVAL, "clrrt_path_device failed");
  v.d_nodes = (clrrt_node*)dn;
  x->pst[0]++;
  // the n headers, read once: the hash, the rows to take and the ranks they come from
  if (v.n > x->h_nodes_cap) {
    const int cap = std::max(v.n, std::max(64, 2 * x->h_nodes_cap));
    x->h_nodes_cap = 0;
    XHIP(x->mem.renew_host(&x->h_nodes, cap));
    x->h_nodes_cap = cap;
  }
  auto read_headers = [&]() -> int {
    if (v.n == 0) return CLRRT_OK;
    XHIP(hipMemcpyAsync(x->h_nodes, v.d_nodes, sizeof(clrrt_node) * v.n, hipMemcpyDeviceToHost, st));
    XHIP(hipEventRecord(x->ev_sum, st));
    XHIP(hipEventSynchronize(x->ev_sum));  // the completion's host wait
    return CLRRT_OK;
  };
  int rc = read_headers();
  if (rc != CLRRT_OK) {
    if (x->group) x->group->rv.abandon();
    return rc;
  }
  for (int i = 0; i < v.n; i++) {
    const clrrt_node& h = x->h_nodes[i];
    if (h.owner == x->rank || h.owner < 0 || h.owner >= x->world || h.nrows < 1) continue;
    v.moved += h.nrows;
    v.need[h.owner] = true;
  }
  PathHdr mine{};
  mine.n = v.n;
  mine.rows = v.rows;
  mine.hash = path_hash(x->h_nodes, v.n);
  rc = x->group ? path_local(x, v, mine, st) : path_rccl(x, v, mine, st);
  if (rc != CLRRT_OK) return rc;
  x->pst[3] += v.moved;
  if (rows_moved) *rows_moved = v.moved;
  return CLRRT_OK;
}

int clrrt_xchg_path_stats(clrrt_xchg* x, int64_t out[4]) {
  if (!x || !out) return fail(CLRRT_EINVAL, "clrrt_xchg_path_stats: null argument");
  memcpy(out, x->pst, sizeof(x->pst));
  return CLRRT_OK;
}

int clrrt_xchg_unique_id(void* out) {
  static_assert(sizeof(ncclUniqueId) == CLRRT_XCHG_UID_BYTES, "the unique id is 128 bytes");
  if (!out) return fail(CLRRT_EINVAL, "clrrt_xchg_unique_id: null pointer");
  ncclUniqueId id;
  XNCCL(ncclGetUniqueId(&id));
  memcpy(out, &id, sizeof(id));
  return CLRRT_OK;
}

int clrrt_xchg_create_rccl(const void* uid, int32_t rank, int32_t world, int32_t device, int32_t cap_records,
                           int32_t first_bound, clrrt_xchg** out) {
  int rc = check_create(rank, world, device, cap_records, first_bound, out);
  if (rc != CLRRT_OK) return rc;
  *out = nullptr;
  if (!uid) return fail(CLRRT_EINVAL, "clrrt_xchg_create_rccl: null unique id");
  std::unique_ptr<clrrt_xchg, void (*)(clrrt_xchg*)> x(new clrrt_xchg, clrrt_xchg_destroy);
  x->rank = rank; x->world = world; x->device = device; x->cap = cap_records;
  x->bound = x->st[6] = std::min<int64_t>(cap_records, first_bound);
  if ((rc = alloc_common(x.get())) != CLRRT_OK) return rc;
  ncclUniqueId id;
  memcpy(&id, uid, sizeof(id));
  XNCCL(ncclCommInitRank(&x->comm, world, id, rank));
  *out = x.release();
  return CLRRT_OK;
}

int clrrt_xchg_group_create(int32_t world, int32_t timeout_ms, clrrt_xchg_group** out) {
  if (!out || world < 1 || world > MAXW || timeout_ms < 1)
    return fail(CLRRT_EINVAL, "clrrt_xchg_group_create: 1 <= world <= 64, timeout_ms >= 1, a non-null result pointer");
  *out = new clrrt_xchg_group(world, timeout_ms);
  return CLRRT_OK;
}

void clrrt_xchg_group_destroy(clrrt_xchg_group* g) { delete g; }

int clrrt_xchg_create_local(clrrt_xchg_group* g, int32_t rank, int32_t device, int32_t cap_records,
                            int32_t first_bound, clrrt_xchg** out) {
  if (!g) return fail(CLRRT_EINVAL, "clrrt_xchg_create_local: null group");
  int rc = check_create(rank, g->rv.world(), device, cap_records, first_bound, out);
  if (rc != CLRRT_OK) return rc;
  *out = nullptr;
  {
    std::lock_guard<std::mutex> lk(g->m);
    if (g->slot[rank].x) return fail(CLRRT_EINVAL, "clrrt_xchg_create_local: the rank exists already");
  }
  std::unique_ptr<clrrt_xchg, void (*)(clrrt_xchg*)> x(new clrrt_xchg, clrrt_xchg_destroy);
  x->rank = rank; x->world = g->rv.world(); x->device = device; x->cap = cap_records;
  x->bound = x->st[6] = std::min<int64_t>(cap_records, first_bound);
  if ((rc = alloc_common(x.get())) != CLRRT_OK) return rc;
  XHIP(hipEventCreateWithFlags(&x->ev_sent, hipEventDisableTiming));
  XHIP(hipEventCreateWithFlags(&x->ev_pulled, hipEventDisableTiming));
  std::lock_guard<std::mutex> lk(g->m);
  if (g->slot[rank].x) return fail(CLRRT_EINVAL, "clrrt_xchg_create_local: the rank exists already");
  x->group = g;
  g->slot[rank].x = x.get();
  *out = x.release();
  return CLRRT_OK;
}

int32_t clrrt_xchg_hook(void* user, clrrt_exchange_io* io) {
  clrrt_xchg* x = (clrrt_xchg*)user;
  if (!x || !io) return fail(CLRRT_EINVAL, "clrrt_xchg_hook: null argument");
  if (io->n_local < 0 || io->n_local > x->cap)
    return fail(CLRRT_ECAPACITY, "clrrt_xchg_hook: n_local outside the send buffer");
  hipStream_t st = (hipStream_t)io->stream;
  const bool closing = (io->flags & 1) != 0;
  x->stream = st;  // the path completion queues its work here
  x->have_stream = true;
  x->st[0]++;
  x->st[3] += closing;
  x->st[4] += io->n_local;
  // the header row (the staging word is free: the last exchange waited for its summary, queued behind its copy)
  Header& h = *x->h_hdr;
  h.n = io->n_local;
  h.elapsed = io->elapsed_ms;
  h.aux = io->aux_local;
  for (int q = 0; q < 4; q++) h.bbox[q] = io->bbox_local[q];
  XHIP(hipMemcpyAsync(x->send, x->h_hdr, sizeof(Header), hipMemcpyHostToDevice, st));
  const int rc = x->group ? hook_local(x, io, st, closing) : hook_rccl(x, io, st, closing);
  if (rc != CLRRT_OK) fprintf(stderr, "clrrt_xchg_hook (rank %d): %s\n", x->rank, t_err.c_str());
  return rc == CLRRT_OK ? 0 : -1;
}

int clrrt_xchg_attach(clrrt_xchg* x, clrrt_ctx* ctx) {
  if (!x || !ctx) return fail(CLRRT_EINVAL, "clrrt_xchg_attach: null argument");
  const int rc = clrrt_set_shards(ctx, x->rank, x->world, x->send + ROW, (int32_t)x->cap, clrrt_xchg_hook, x);
  if (rc != CLRRT_OK) return fail(rc, std::string("clrrt_set_shards: ") + clrrt_last_error(ctx));
  x->ctx = ctx;
  return CLRRT_OK;
}

void* clrrt_xchg_records(clrrt_xchg* x) { return x ? (void*)(x->send + ROW) : nullptr; }

int clrrt_xchg_stats(clrrt_xchg* x, int64_t out[8]) {
  if (!x || !out) return fail(CLRRT_EINVAL, "clrrt_xchg_stats: null argument");
  memcpy(out, x->st, sizeof(x->st));
  return CLRRT_OK;
}

void clrrt_xchg_destroy(clrrt_xchg* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  if (x->group) {
    std::lock_guard<std::mutex> lk(x->group->m);
    if (x->group->slot[x->rank].x == x) x->group->slot[x->rank].x = nullptr;
  }
  if (x->comm) (void)ncclCommDestroy(x->comm);
  x->mem.release_all();
  for (hipEvent_t e : {x->ev_sum, x->ev_sent, x->ev_pulled})
    if (e) (void)hipEventDestroy(e);
  delete x;
}

int clrrt_xchg_selftest_concat(int32_t device, int32_t W, int32_t bound, const int32_t* counts, const double* elapsed,
                               const int64_t* aux, const double* bbox, int32_t excess_rows, void* out_rows,
                               int64_t out_cap, int64_t* summary) {
  if (W < 1 || W > MAXW || bound < 1 || device < 0 || excess_rows < 0 || !counts || !elapsed || !aux || !bbox ||
      !summary || out_cap < 0 || (out_cap > 0 && !out_rows))
    return fail(CLRRT_EINVAL, "clrrt_xchg_selftest_concat: bad argument");
  int64_t total = 0;
  for (int r = 0; r < W; r++) {
    if (counts[r] < 0 || counts[r] > (int64_t)bound + excess_rows)
      return fail(CLRRT_EINVAL, "clrrt_xchg_selftest_concat: a count outside [0, bound + excess_rows]");
    total += counts[r];
  }
  if (total > out_cap) return fail(CLRRT_EINVAL, "clrrt_xchg_selftest_concat: out_cap < sum(counts)");
  const int64_t stride = (int64_t)bound + 1;
  std::vector<unsigned char> hp((size_t)W * stride * ROW), hx((size_t)W * excess_rows * ROW);
  for (int r = 0; r < W; r++) {
    for (int64_t j = 0; j < (int64_t)bound + excess_rows; j++) {
      unsigned char* row = j < bound ? &hp[((size_t)r * stride + 1 + j) * ROW]
                                     : &hx[((size_t)r * excess_rows + (j - bound)) * ROW];
      for (int b = 0; b < ROW; b++) row[b] = (unsigned char)(r * 131 + j * 7 + b * 3 + 1);
    }
    Header h;
    h.n = counts[r];
    h.elapsed = elapsed[r];
    h.aux = aux[r];
    for (int q = 0; q < 4; q++) h.bbox[q] = bbox[4 * r + q];
    memset(&hp[(size_t)r * stride * ROW], 0, ROW);
    memcpy(&hp[(size_t)r * stride * ROW], &h, sizeof(h));
  }
  XHIP(hipSetDevice(device));
  Scratch<char> dp, dx, dout;
  Scratch<Summary> ds;
  Summary hs;
  XHIP(dp.alloc(hp.size()));
  XHIP(dx.alloc(std::max<size_t>(hx.size(), 16)));
  XHIP(dout.alloc(std::max<size_t>((size_t)total * ROW, 16)));
  XHIP(ds.alloc(1));
  XHIP(hipMemcpy(dp, hp.data(), hp.size(), hipMemcpyHostToDevice));
  if (!hx.empty()) XHIP(hipMemcpy(dx, hx.data(), hx.size(), hipMemcpyHostToDevice));
  XHIP(hipMemset(dout, 0, std::max<size_t>((size_t)total * ROW, 16)));
  ConcatArgs a{};
  a.parts = (const uint4*)dp.p;
  a.excess = excess_rows > 0 ? (const uint4*)dx.p : nullptr;
  a.out = (uint4*)dout.p;
  a.summary = ds;
  a.part_stride = stride;
  a.ex_stride = a.ex_rows = excess_rows;
  a.out_cap = total;
  a.cap_rows = (int64_t)bound + excess_rows;
  a.W = W;
  a.bound = bound;
  a.copy_first = a.copy_excess = 1;
  XHIP(launch_concat(nullptr, a, (int64_t)bound + excess_rows));
  XHIP(hipDeviceSynchronize());
  if (total > 0) XHIP(hipMemcpy(out_rows, dout, (size_t)total * ROW, hipMemcpyDeviceToHost));
  XHIP(hipMemcpy(&hs, ds, sizeof(hs), hipMemcpyDeviceToHost));
  summary[0] = hs.n_all;
  summary[1] = hs.max_count;
  memcpy(&summary[2], &hs.max_elapsed, 8);
  summary[3] = hs.aux_sum;
  memcpy(&summary[4], hs.bbox, 32);
  for (int r = 0; r < W; r++) summary[8 + r] = hs.counts[r];
  return CLRRT_OK;
}

int clrrt_xchg_selftest_path_select(int32_t device, int32_t W, int32_t self, int32_t n, const int32_t* owners,
                                    const int32_t* nrows, void* out_rows, int64_t* out_moved) {
  if (W < 1 || W > MAXW || self < 0 || self >= W || device < 0 || n < 0 || !out_moved || (n > 0 && (!owners || !nrows)))
    return fail(CLRRT_EINVAL, "clrrt_xchg_selftest_path_select: bad argument");
  std::vector<clrrt_node> hn((size_t)n);
  int64_t R = 0, moved = 0;
  for (int i = 0; i < n; i++) {
    if (owners[i] < 0 || owners[i] >= W || nrows[i] < 1)
      return fail(CLRRT_EINVAL, "clrrt_xchg_selftest_path_select: an owner outside [0, W) or a node without rows");
    memset(&hn[i], 0, sizeof(clrrt_node));
    hn[i].nrows = nrows[i];
    hn[i].owner = owners[i];
    hn[i].row_offset = R;
    R += nrows[i];
    if (owners[i] != self) moved += nrows[i];
  }
  *out_moved = 0;
  if (R > 0 && !out_rows) return fail(CLRRT_EINVAL, "clrrt_xchg_selftest_path_select: null out_rows");
  std::vector<uint64_t> hp((size_t)W * R * 10);
  for (int r = 0; r < W; r++)
    for (int64_t j = 0; j < R; j++)
      for (int c = 0; c < 10; c++) {
        const uint64_t b = ((uint64_t)(r + 1) << 44) | ((uint64_t)j << 8) | (uint64_t)c;
        uint64_t v = b;
        switch ((j + c) % 5) {
          case 1: v = 0x7FF8000000000000ull | b; break;
          case 2: v = 0xFFF0000000000000ull | b; break;
          case 3: v = 0x8000000000000000ull; break;
          case 4: v = 0x4000000000000000ull | b; break;
          default: break;
        }
        hp[((size_t)r * R + j) * 10 + c] = v;
      }
  XHIP(hipSetDevice(device));
  const size_t part = (size_t)R * PROW;
  Scratch<char> dp, dd;
  Scratch<clrrt_node> dn;
  XHIP(dp.alloc(std::max<size_t>(part * W, 16)));
  XHIP(dd.alloc(std::max<size_t>(part, 16)));
  XHIP(dn.alloc(n));
  if (R > 0) {
    XHIP(hipMemcpy(dp, hp.data(), part * W, hipMemcpyHostToDevice));
    XHIP(hipMemcpy(dd, hp.data() + (size_t)self * R * 10, part, hipMemcpyHostToDevice));  // its own pattern
    XHIP(hipMemcpy(dn, hn.data(), sizeof(clrrt_node) * n, hipMemcpyHostToDevice));
  }
  PathSelectArgs a{};
  a.parts = (const uint4*)dp.p;
  a.dst = (uint4*)dd.p;
  a.nodes = dn;
  a.rows = R;
  a.n = n;
  a.W = W;
  a.self = self;
  XHIP(launch_path_select(nullptr, a));
  XHIP(hipDeviceSynchronize());
  if (R > 0) XHIP(hipMemcpy(out_rows, dd, part, hipMemcpyDeviceToHost));
  *out_moved = moved;
  return CLRRT_OK;
}

}  // extern "C"
