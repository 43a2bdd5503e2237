// clrrt_capi.hip — host side of libclrrt: the C-ABI of include/clrrt.h.
//
// Round structure of one batch of expandTree iterations (rrtplanner.cpp:123-174) on the GPU:
//   1. nearest-node search for every sample against the frozen tree        (k_nn_partial/merge)
//   2. every candidate rollout of every sample, speculatively in parallel; a successful candidate
//      that passes the goal-bias gate continues in the same lane with the goal-biased rollout;
//      rows go to per-job slots                                              (k_rollout SPEC)
//   3. first success per sample -> regular node (+ goal-biased node)         (k_select)
//   4. EXACT mode only: first sample whose candidate list a node of an earlier sample of the round
//      would reorder (k_conflict) -> commit the prefix before it, re-draw nothing, retry the rest
//   5. scan committed samples -> node records, arena offsets, counters       (k_compact)
//   6. copy the accepted trajectories from their slots into the arena        (k_copy_rows)
//   7. append the records to the tree                                        (k_append)
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <climits>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <optional>
#include <string>
#include <vector>

#include "../../include/clrrt.h"
#include "clrrt_dev.hpp"
#include "clrrt_devmem_hip.hpp"
#include "clrrt_internal.hpp"

static const int kWalkMaxOver = 2048, kWalkMaxChunks = 64;  // walk overflow records, split waves per record

using namespace clrrt;

#define CAND_K 10
#define NN_K 11

// One round's samples and candidate lists.  The context keeps three sets and names them by role (clrrt_ctx::ls).
struct ListSet {
  clrrt_sample* d_samples = nullptr;  // [max_batch]
  clrrt_sample* h_samples = nullptr;  // [max_batch] pinned
  int* cand = nullptr;                // [max_batch * CAND_K]
  float* ckey = nullptr;              // [max_batch * CAND_K]
  int* ncand = nullptr;               // [max_batch]
  int* ctie = nullptr;                // [max_batch]
  // lag-2 rounds only (lag_alloc)
  hipEvent_t ev = nullptr;   // recorded after the set's merge
  hipEvent_t evw = nullptr;  // recorded after its walk (the merge waits for it on the merge stream)
  hipEvent_t evm = nullptr;  // recorded after the walk's main grid (and wseed)
  float* wseed = nullptr;    // [max_batch] the appended-node search's caps, taken after the main grid
};

// Search region (the sampling region and the tree's box) and the float frame of the searches.
struct NnSetup {
  NnFrame fr;
  double x0, y0, x1, y1;
  bool region_ok;
};

// What a walk index was built for (n = -1: nothing): the tree size, the node range, the frame and region, the index
// options.  Nodes never change once appended, so an index stays valid while all of these are the same.
struct BuiltFor {
  int64_t n = -1, first = 0, count = 0;
  double ox = 0, oy = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  float delta = 0;
  int kind = 0, hscale = 0;
  void set(int64_t n_, int64_t first_, int64_t count_, const NnSetup& su, int kind_, int hscale_) {
    n = n_; first = first_; count = count_;
    ox = su.fr.ox; oy = su.fr.oy; delta = su.fr.delta;
    x0 = su.x0; y0 = su.y0; x1 = su.x1; y1 = su.y1;
    kind = kind_; hscale = hscale_;
  }
  bool matches(int64_t n_, int64_t first_, int64_t count_, const NnSetup& su, int kind_, int hscale_) const {
    BuiltFor o;
    o.set(n_, first_, count_, su, kind_, hscale_);
    return n == o.n && first == o.first && count == o.count && ox == o.ox && oy == o.oy && delta == o.delta &&
           x0 == o.x0 && y0 == o.y0 && x1 == o.x1 && y1 == o.y1 && kind == o.kind && hscale == o.hscale;
  }
};

struct clrrt_ctx {
  int device = 0;
  int rank = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  clrrt_params params;
  DevParams dp;
  clrrt_capacity cap;
  std::string err;
  // Every device and pinned buffer below (and in the WalkBufs, ListSet, def and sh groups) is allocated through `mem`
  // (renew / renew_host) and freed by it: free_all's release_all, after the streams have drained.
  clrrt::DevMem<HipMem> mem;
  // tree
  clrrt_node* tree = nullptr;
  NnRec* nn = nullptr;
  double* arena = nullptr;
  int64_t n_nodes = 0, n_rows = 0;
  bool tree_rowless = false;  // the tree came from clrrt_tree_load: its first nodes have no rows in the arena
  int64_t rebase_window_rows = 786432;  // option "rebase_window_rows": clrrt_tree_rebase's move window (60 MiB)
  // obstacles
  BakedObs* obs = nullptr;
  int n_obs = 0;
  ObsGrid grid{};              // device view of the static-obstacle grid
  void* grid_buf = nullptr;    // start | items | mov
  size_t grid_bytes = 0;
  int grid_exempt = 0;         // obstacles exempt from culling (always-tested list, see build_grid)
  // the static occupancy grid (CLRRT_COLLISION_OCC, clrrt_set_occupancy): the baked maps' device view (w == 0:
  // none), their buffer (cell bytes | counts | occ words | reach words | union reach words, each but the counts once
  // per layer of a stack), the occupied count (all layers, and per layer) and the bake's events
  OccGrid occ{};
  void* occ_buf = nullptr;
  size_t occ_bytes = 0;
  int64_t occ_count = 0;
  int64_t occ_counts[CLRRT_OCC_MAX_LAYERS] = {};
  hipEvent_t occ_ev[2] = {nullptr, nullptr};
  float occ_bake_ms = 0.f;
  // the occupancy clearance (clrrt_set_occupancy_clearance): its cap (0: off), the field's buffer (field dwords | row
  // distances | row mask; occ.field points into it while a field is baked) and the field bake's events
  double clr_max = 0.0;
  void* clr_buf = nullptr;
  size_t clr_bytes = 0;
  hipEvent_t clr_ev[2] = {nullptr, nullptr};
  float clr_bake_ms = 0.f;
  // round buffers (capacity cap.max_batch samples)
  // The list sets: sets[] holds the buffers (sets 0 and 1 from clrrt_create, set 2 and the lag-2 members of all three
  // from lag_alloc), ls[] names them by role: ls[0] this round's set, ls[1] the set the
  // side stream searches for the next round (lag 2: round r+1's, being merged), ls[2] lag 2's round r+2's, being
  // searched.  ls[] is a permutation of &sets[0..2] at every instant, so any exit leaves a context safe to free and
  // to reuse.
  ListSet sets[3];
  ListSet* ls[3] = {&sets[0], &sets[1], &sets[2]};
  float* pk = nullptr;
  int* pi = nullptr;
  int64_t partial_cap = 0;  // entries (samples * chunks * K)
  KeyId* sort_scratch = nullptr;
  int64_t sort_cap = 0;  // KeyId entries
  RollRes* res_spec = nullptr;
  clrrt_node* regnodes = nullptr;
  RollRes* res_gb = nullptr;
  double* slots = nullptr;  // rollout rows of one round, [2][max_batch * CAND_K][slot_rows][10] (allocated
                            // only when rows are not deferred: option "rows_deferred" 0 or the non-persistent path)
  int slot_rows = 0;
  // deferred rows (option "rows_deferred", default 1): the persistent rollouts store no rows; each commit
  // gathers its accepted rollouts' start states into rep_buf and the next persistent launch replays them
  // into the arena (flush_replays runs them alone when rows are needed before that)
  int rows_deferred = 1;
  void* rep_buf = nullptr;  // [2 max_batch] Replay
  int rep_n = 0;            // pending replays
  bool eval_deferred = false;  // the last eval_samples ran with deferred rows
  clrrt_node* gbnodes = nullptr;
  SampleOut* so = nullptr;
  int* first_conflict = nullptr;
  clrrt_node* out_nodes = nullptr;
  Job* jobs = nullptr;
  int64_t* totals = nullptr;
  bool totals_zeroed = false;  // the round's prologue fill reset totals (launch_compact skips its own fill)
  unsigned long long* work_ctr = nullptr;  // [3] algorithmic rollout work; [8..15] nn search statistics
  // spatial index of the tree (nearest-node search)
  float* nn_seed = nullptr;  // [max_batch] the brute-force chunks' shared per-sample key caps
  // bounding box of the tree's finite node positions (x0, y0, x1, y1), maintained on the host
  double bbox[4] = {HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  double* d_bbox = nullptr;  // [4] device result of launch_bbox
  double* h_bbox = nullptr;  // [4] pinned
  int64_t nnw_min_nodes = 8192;       // walk search (clrrt_nnwalk.hip) from this tree size ("nn_walk_min")
  bool nnw_stateless = false;          // "nn_walk_stateless": the large-tree variant at every size (tests)
  // walk overflow ("nn_walk_budget_tiles", "nn_walk_budget_keys", 0 = off; "nn_walk_chunks" <= 64;
  // "nn_walk_max_over" records <= 2048); defaults from the cfg3 bench sweeps (round 3
  // with lag 2: 3072 tiles 1.039 vs 2048 1.031 M nodes/s, 8192 keys 1.008, 12 chunks 1.030)
  int nnw_bud_tiles = 3072, nnw_bud_ex = 4096, nnw_chunks = 16, nnw_max_over = 1024;
  // "nn_walk_max_over" unset: 1024 records, 2048 on trees of >= 6 Mi nodes (at 8 M nodes 1024 records ran out
  // and the samples past them searched alone: 31.7 -> 24.1 ms per 16384-sample round, profiles/r04u)
  bool nnw_max_over_set = false;
  // "nn_walk_budget_tiles" unset: max(3072, N / 2048) tiles (16 M nodes: 3072 overflowed 2048 samples per
  // round, 8192 -> 45.6 vs 58-59 ms; 8 M: 3072 stays best, 25.8 vs 29.9 ms at 8192, profiles/r04as)
  bool nnw_bud_tiles_set = false;
  int nnw_half_max = 4096;  // option "nn_walk_half_max": super-tiles up to which the walk keeps fp16 LDS bounds
  // option "nn_walk_hscale": the 3D index codes' heading axis, percent of rho per radian (round 6: 25 / 50 / 100 / 200
  // -> cfg3 1.289 / 1.293 / 1.274 / 1.232 M nodes/s, profiles/r06k_*)
  int nnw_hscale = 50;
  int nnw_root_seed = 1;    // option "nn_root_seed": optimize samples start from the root roster (WalkBufs::roster)
  int nnw_root_k = 64;      // option "nn_root_k": roster entries
  int nnw_root_scan = 16384;  // option "nn_root_scan": ids scanned for them
  int nnw_index = 5;       // option "nn_walk_index": the index's place order (WalkBufs::index_kind); 5 since round 6
  // option "nn_walk_waves": the walk's persistent grid (waves taking samples from per-XCD counters; 0 = one
  // wave per sample; -1, the default: 9 per CU).  A fixed grid leaves wave slots to the kernels that run
  // beside the lag-2 walk (the commit's k_select waited ~1.2 ms per round for slots behind ~1 ms walk waves)
  // and balances the walk's own tail: cfg3 1.164 -> 1.203 M nodes/s (round 4 sweep: 1024 / 1536 / 2048 /
  // 2560 waves -> 1.07 / 1.17 / 1.202 / 1.203 M), the 16 M-node search alone 62 -> 58 ms at 3072; the default
  // grid is used for batches of >= 4x its waves (below, one wave per sample).  Round 6: 8 per CU -- with the
  // rollout waves at 320 registers a walk wave fits beside them, and the rollout kernel gains more from the slots a
  // smaller walk grid leaves than the walk loses (cfg3, kind 5: 1536 / 1792 / 2048 / 2304 / 2560 waves -> 1.238 /
  // 1.257 / 1.275 / 1.256 / ~1.23 M nodes/s, profiles/r06i_*); then 9 per CU with the walk kernels at 96 VGPRs
  // (CLRRT_WALK_WAVES 5, clrrt_nnwalk.hip: two walk waves fit beside a rollout wave; 2048 / 2304 / 2560 / 2816 /
  // 3072 waves -> 1.285 / 1.310, 1.306 / 1.292, 1.303 / 1.287, 1.288 / 1.269 M against 1.288-1.290 M for the
  // 128-VGPR walk at 2048, profiles/r06r_*, r06s_*)
  int nnw_waves = -1;
  int nnw_double = 1;  // "nn_walk_double": build the next round's index while the side search runs
  WalkBufs nnw{};                      // allocated on first use
  // pipelined rounds: a second index set, so the next round's index is built while the side stream's
  // search still reads this one (swapped in after each commit); nnw_built: what the current set's index
  // was built for (the whole tree: tree_index_matches)
  WalkBufs nnw_alt{};
  BuiltFor nnw_built;
  CompactBufs cmp{};                   // round compaction scratch
  // persistent rollouts (k_roll_run; k_roll_flag + k_roll_order for the queue order)
  int roll_persistent = 1;
  int nn_debug = 0;
  int roll_blocks = 0;       // persistent blocks (0: 5/8 of the CUs)
  int n_cu = 256;
  int* roll_q = nullptr;      // [1] queue head
  int* roll_best = nullptr;   // [max_batch] first successful candidate per sample
  int roll_priority = 1;      // option "roll_priority": longest-predicted chains first (k_roll_order)
  int roll_order_verify = 0;  // option "roll_order_verify" (diagnostics): check the order, work counters 6 / 7
  int roll_coop = 1;          // option "roll_coop": wave-cooperative collision checks in k_roll_run
  int roll_spread = 1;        // option "roll_spread": a short queue is spread over the persistent waves
  int roll_lanes = 0;         // option "roll_lanes": lanes per wave that take jobs (0: 64, or fewer by roll_spread)
  int nn_exact_fused = 1;     // option "nn_exact_fused": EXACT lists of small trees by k_nn_exact_fused
  int exact_min_width = 8;    // option "exact_min_width": EXACT rounds speculate at least this many samples
  // option "exact_fixup" (default 1): EXACT rounds resolve a conflict by rolling out the conflicting new nodes for
  // the sample (k_conflict_fix) instead of ending the committed prefix there, when that decides it
  int exact_fixup = 1;
  // option "exact_fixup_cap": fix-up rollouts run at most this many steps (0: to their end); one that reaches it is
  // undecided and ends the prefix at its sample (re-evaluated next round), so a round never waits for a long one
  int exact_fix_cap = 0;
  int* fix_n = nullptr;        // [max_batch]
  int* fix_ids = nullptr;      // [max_batch * FIX_MAX]
  int* fix_adj = nullptr;      // [max_batch * FIX_ADJ]
  NnRec* fix_xrec = nullptr;   // [2 max_batch] the round's new nodes as nearest-node records
  int* fix_xi = nullptr;       // [2 max_batch] samples whose list is recomputed, their new-node counts
  int* fix_xcand = nullptr;    // [max_batch * K] recomputed lists
  float* fix_xkey = nullptr;   // [max_batch * K]
  int* fix_xn = nullptr;       // [2 max_batch] list lengths, tie flags
  std::vector<int> h_fix_cand;
  std::vector<RollRes> h_fix_spec;
  Job* fix_jobs = nullptr;     // [max_batch * CAND_K]
  RollRes* fix_res = nullptr;  // [max_batch * CAND_K]
  std::vector<int> h_fix;      // fix_n, fix_ids, then fix_adj
  std::vector<clrrt_sample> h_fix_smp;
  std::vector<Job> h_fix_jobs;
  std::vector<int> h_fix_owner;
  std::vector<RollRes> h_fix_res;
  std::vector<SampleOut> h_fix_so;
  // EXACT: rounds, conflicts resolved, fix-up rollouts, rounds ended by a conflict; then why the ending conflicts
  // were not resolved: a fix-up succeeded, tie, key equal to the threshold, > FIX_MAX nodes, k pushed out, full
  // window without a result
  int64_t ex_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // clrrt_exact_fix_hist: the verdicts of exact_fixups per sample of each round's committed prefix and the sample that
  // ended it (the buckets of include/clrrt.h), on either side of the recomputed lists' size limit
  int64_t ex_hist[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int* roll_perm = nullptr;   // [max_batch * CAND_K] queue order
  int* roll_pflag = nullptr;  // [roll_order_ints(max_batch * CAND_K)] length classes, block histograms, verify marks
  // extractBestPath scratch (allocated on first use, max_nodes entries each)
  GoalRec* goal_recs = nullptr;
  int* bp_path = nullptr;  // [max_nodes + 2]: chain, then count and length
  // committed path (MotionPlanner::bestNodes) + initializeTree scratch
  clrrt_node* path_nodes = nullptr;
  double* path_rows = nullptr;
  int path_cap = 0;
  int64_t path_rows_cap = 0;
  int path_n = 0;
  int64_t path_nrows = 0;
  int* ri_int = nullptr;       // [2 * path_cap + ...] ids, kept index, goal flags
  int64_t* ri_off = nullptr;   // [path_cap] new row offsets, then [3] outcome / nodes / rows
  float* ri_cost = nullptr;    // [path_cap]
  double* ri_terms = nullptr;  // [2 * path_rows_cap]
  double reg_x0 = 0, reg_y0 = 0, reg_x1 = 0, reg_y1 = 0;  // sampling region + margin
  // pipelined BATCH rounds (clrrt_expand): while a round's rollouts run on `stream`, the walk search
  // of the next round's samples over the same tree runs on `side` into the set ls[1]; the round
  // then merges in the nodes it appended (launch_nn_delta) and ls[0] / ls[1] swap
  int nn_pipeline = 1;  // option "nn_pipeline"
  hipStream_t side = nullptr;
  hipEvent_t ev_tree = nullptr, ev_walk = nullptr, ev_commit = nullptr;
  // option "nn_lag" (1 or 2; 0 = by query length): how many rounds ahead the pipelined BATCH rounds search
  // (2: expand_lag2).  The default picks 2 for long queries (a budget of >= 1 s or >= 64 rounds), 1 for
  // short ones: round-3 A/B, cfg3 (2 s) 1.031 vs 1.015 M nodes/s for lag 2; cfg2 (200 ms) 0.551 vs 0.565 M
  // for lag 1; cfg5 (200 ms) equal.  (With round 2's rollout kernel lag 1 was ahead on cfg3 too.)
  // Lag 2 keeps a third list set (ls[2]), a third walk index set and a second side stream (allocated on
  // first use).
  int nn_lag = 0;
  WalkBufs nnw3{};
  hipStream_t side2 = nullptr;
  // lag 2: the appended-node merges run on their own stream (mst), behind the commit and the slot's walk
  // (its set's event evw); with option "stream_prio" (default 1) the main and merge streams have the device's
  // highest priority and the walk streams (side, side2) its lowest, so the commit and merge kernels are
  // not queued behind thousands of walk waves (kernel trace: k_select 16 us -> 1.9 ms late in a query)
  hipStream_t mst = nullptr;
  // (Round 6 also split the appended-node search by commit, option "nn_split_delta": the lists were the same and the
  // round no faster -- the GPU is work-bound there, profiles/r06o_* -- so the path is gone.)
  // option "nn_delta_walk" (default 1): the lag-2 appended-node search walks a place-ordered index of the appended
  // range (launch_nn_delta_walk, buffer set nnw_d) instead of brute-forcing every (sample, appended node) pair
  // (k_nn_partial: 0, and the fallback where the walk's preconditions fail).  Same lists either way.
  int nn_delta_walk = 1;
  // option "nn_delta_verify" (diagnostics, default 0): every appended-node walk is followed by the brute force over
  // the same range and caps, and k_nn_delta_compare counts the samples compared / differing in work counters 38 / 39
  // (the walk's own statistics go to counters 40..52, the brute force's queued pairs and exact keys to 54 / 55).
  int nn_delta_verify = 0;
  WalkBufs nnw_d{};
  // Tree-partitioned search (clrrt_nn_range): the walk over a node range [first, first + count) of any size has an
  // index set of its own (a full set, allocated on first use; launch_nn_walk_build with a node-id base), so the sets
  // of the pipelined rounds (nnw, nnw_alt, nnw3, nnw_d) stay as they are.  nnr_built: what its index was built for;
  // every call that replaces or drops nodes goes through pf_reset, which clears it.
  WalkBufs nnw_r{};
  BuiltFor nnr_built;
  // clrrt_nn_merge's inputs on the device ([part][sample][CAND_K] ids / keys, [part][sample] counts; grown on demand)
  int* pm_ids = nullptr;
  float* pm_keys = nullptr;
  int* pm_counts = nullptr;
  int64_t pm_cap = 0;    // (part, sample) pairs the three hold
  int* d_bad = nullptr;  // [1] clrrt_round_eval_lists: the first sample whose list fails the check
  float* vpk = nullptr;    // nn_delta_verify: the brute force's chunk lists (partial_cap entries) ...
  int* vpi = nullptr;
  float* vseed = nullptr;  // ... and its copy of the caps (k_nn_partial lowers them)
  // Lag 2 (round 6): the appended-node search of a slot starts after its walk's main grid (key caps from k_walk_seed,
  // in the set's wseed), not after the overflow split and its merge, so it runs beside the split (a cfg3 trace: main
  // grid done 1.7 ms before the rollout kernel, split until 0.6 ms after it, the search after that until 1.9 ms,
  // profiles/r06w_cfg3_list_crit.txt); the merge still waits for the whole walk.  Its brute-force fallback puts
  // optimize samples on their own lanes (k_nn_order, nn_order), so explore lanes do not idle while optimize lanes
  // compute exact keys.
  int* nn_order = nullptr;  // [max_batch]
  int stream_prio = 1;
  bool stream_prio_applied = false;  // the lag-2 streams have stream_prio's priorities (false: all the default one)
  // clrrt_round_prefetch: declared next samples; pf_state 1 = their walk was launched (lists in the
  // set ls[1], merge pending), 2 = merged and swapped in for pf_samples
  std::vector<clrrt_sample> pf_next, pf_samples;
  int pf_state = 0;
  // Deferred samples (BATCH option "defer_steps" T > 0; see Carry in clrrt_kernels.hip): every rollout chain
  // runs at most T more steps per launch; suspended chains resume at the front of the next launch and a
  // sample commits at the first commit after which nothing its result depends on is still running.  The
  // per-job results, lists and first-success flags of the rounds in flight live in rings of R round slots
  // (a chain of at most 2 n_steps_max steps resolves within ceil(2 n_steps_max / T) launches, so a slot is
  // free again when the ring comes round); the commit buffers hold vcap views (deferred + this round's).
  struct {
    int T = 0;                    // option value (0: off)
    bool active = false;          // the current expansion defers
    int R = 0;                    // ring slots allocated (for T_alloc / n_steps_alloc)
    int T_alloc = 0, n_steps_alloc = 0;
    int64_t vcap = 0;             // views the commit buffers hold
    RollRes* res = nullptr;       // [R][B][K]
    RollRes* res_gb = nullptr;    // [R][B][K]
    int* cand = nullptr;          // [R][B][K]
    int* ncand = nullptr;         // [R][B]
    clrrt_sample* samp = nullptr; // [R][B]
    int* best = nullptr;          // [R][B]
    int* dlist[2] = {nullptr, nullptr};  // ring indices of the deferred samples (views 0 .. nd)
    int cur_dl = 0, nd = 0;
    int nd_eval = -1;             // nd when the current round's views were selected (-1: no views)
    int* gv = nullptr;            // [vcap]
    uint8_t* pend = nullptr;      // [vcap]
    void* sel_tmp = nullptr;
    size_t sel_bytes = 0;
    int* d_cnt = nullptr;         // [3] selected views, suspended chains, this round's samples left pending (device)
    void* carry[2] = {nullptr, nullptr};
    int cur_c = 0, ncarry = 0, carry_cap = 0;
    int64_t round = 0;            // rounds of the current expansion
    int slot = 0;                 // ring slot of the current round
    int64_t deferred_total = 0;   // samples deferred at least once (statistics)
  } def;
  // Sharded BATCH expansion (clrrt_set_shards): this rank's slice of every round, one exchange of the
  // accepted-node records per round through the caller's collective
  struct {
    int rank = 0, world = 1;
    void* dev_local = nullptr;     // the caller's buffer the local records go to
    int cap_local = 0;
    clrrt_exchange_fn fn = nullptr;
    void* user = nullptr;
    double max_ms = 0;             // largest elapsed query time over the ranks at the last exchange
    int64_t nd_global = 0;         // deferred samples pending on all ranks after the last exchange
    int64_t rows_stop = 0;         // ranks whose arena cannot take another round (the same stop everywhere)
    int last_nb = 0;               // this rank's slice of the last round
    clrrt_node* xbuf = nullptr;    // the exchanged records in commit order (deferred samples: by age)
    uint32_t* xkey = nullptr;      // [2 xcap] sort keys (age), [2 xcap] record indices
    void* xtmp = nullptr;
    size_t xtmp_bytes = 0;
    int64_t xcap = 0;
    unsigned long long* d_goal = nullptr;  // goal nodes among the appended records (device counter)
    // errors are collective: a rank that fails sends an error flag through the exchange's aux word (bit 48) in
    // the exchange the other ranks make next -- a round's, or the closing exchange every sharded expansion ends
    // with -- so every rank leaves the expansion instead of waiting in a collective the failed rank never joins
    bool poison_seen = false;      // an exchange of this expansion reported another rank's failure
    bool fn_failed = false;        // the exchange hook itself failed (the collective is broken: no more calls)
    // option "shard_hook_world1": clrrt_set_shards with world 1 keeps dev_local and the hook, and the expansion
    // runs the sharded commit path with one rank (a set hook, not world > 1, is what selects that path)
    bool hook_world1 = false;
  } sh;
  // option "fail_at_round" k (fault injection, tests): the k-th commit from now fails with CLRRT_ECAPACITY
  // after the round's deferred-sample bookkeeping, as the "trajectory arena full" check does
  int fail_at_round = 0;
  // option "fail_after_exchange" k (fault injection, tests): the k-th exchange from now fails after the hook
  // returned (as a failure of the work that follows the round's exchange would)
  int fail_after_exchange = 0;
  // option "fail_in_round" k (fault injection, tests): the k-th round from now fails with CLRRT_ECAPACITY in the
  // driver's round body right after its commit, as a HIP error of the work queued there would (a host-side return)
  int fail_in_round = 0;
  // CLRRT_DEBUG_SYNC (diagnostics, read once at clrrt_create): a heartbeat buffer the rollout kernel's waves
  // write, polled while waiting for the launch
  bool debug_sync = false;
  unsigned long long* dbg_host = nullptr;
  // clrrt_iteration_log: one record per committed iteration (EXACT / non-deferred BATCH rounds)
  bool iter_log = false;
  // the tree size after each commit of the last clrrt_expand (its rounds, then the drain of deferred samples when it
  // appended anything): clrrt_round_sizes
  std::vector<int64_t> round_sizes;
  std::vector<clrrt_iteration> iters;
  std::vector<SampleOut> iter_tmp;
  // host staging (pinned)
  int64_t* h_totals = nullptr;
  int* h_int = nullptr;
  // last round_eval bookkeeping
  int64_t last_eval_rows = 0;
  int64_t last_goal_nodes = 0;
  // counters
  clrrt_counters counters{};
  int64_t nn_bf_keys = 0, nn_samples = 0;  // search work: brute-force-equivalent keys, samples searched
  int64_t nn_super_bounds = 0;             // walk searches' phase-1 super-tile bounds (samples x super-tiles)
  // timing
  bool timing = false;
  // per class: 0 nearest-node search (index builds, walks, merges), 1 rollouts, 2 select / commit,
  // 3 the walk searches alone (launch_nn_walk_search: sample order, k_walk_search, split + merge; within class 0),
  // 4 the main stream's wait for a round's lists (the side streams' walk + merge running past the work queued
  // before it: the search's share of the round's critical path), 5 sharded exchanges (the stream span from the
  // records' copy to the gathered records' availability: the collective on the critical path), 6 clrrt_tree_rebase's
  // check kernel (k_rebase_check alone: its bandwidth basis is rows x 80 B)
  static constexpr int kKtClasses = 7;
  double kt_ms[kKtClasses] = {};
  int64_t kt_n[kKtClasses] = {};
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_pending;
};

// ------------------------------------------------------------------------------------------ util
static void pf_reset(clrrt_ctx* c);
static int flush_replays(clrrt_ctx* c);
static RollArgs roll_args(clrrt_ctx* c, int njobs);
static int append_nodes(clrrt_ctx* c, const clrrt_node* dev_nodes, int n);
static int watchdog_check(clrrt_ctx* c);
static void defer_roll_args(clrrt_ctx* c, RollArgs& a, bool capped);
static int commit_round(clrrt_ctx* c, int nn, double elapsed_ms, int* n_app);
static int ensure_slots(clrrt_ctx* c);

static int fail(clrrt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPC(c, call)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail((c), CLRRT_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)
// as HIPC, for the entry points whose failures read "<entry>: <error>"
#define HIPP(c, prefix, call)                                                                  \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) return fail((c), CLRRT_EHIP, std::string(prefix) + hipGetErrorString(e_)); \
  } while (0)

static hipEvent_t ev_get(clrrt_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

struct KTimer {
  clrrt_ctx* c;
  int which;
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  KTimer(clrrt_ctx* c_, int w, hipStream_t s_ = nullptr) : c(c_), which(w), s(s_ ? s_ : c_->stream) {
    if (!c->timing) return;
    a = ev_get(c);
    b = ev_get(c);
    if (a) hipEventRecord(a, s);
  }
  ~KTimer() {
    if (!c->timing || !a || !b) return;
    hipEventRecord(b, s);
    c->ev_pending.push_back({which, {a, b}});
  }
};

static void drain_timers(clrrt_ctx* c) {
  for (auto& pe : c->ev_pending) {
    float ms = 0;
    hipEventSynchronize(pe.second.second);
    if (hipEventElapsedTime(&ms, pe.second.first, pe.second.second) == hipSuccess) {
      c->kt_ms[pe.first] += ms;
      c->kt_n[pe.first] += 1;
    }
    c->ev_pool.push_back(pe.second.first);
    c->ev_pool.push_back(pe.second.second);
  }
  c->ev_pending.clear();
}

// The grid the kernels test: the baked one under CLRRT_COLLISION_OCC, none otherwise.
static OccGrid occ_view(const clrrt_ctx* c) {
  return c->params.collision_mode == CLRRT_COLLISION_OCC ? c->occ : OccGrid{};
}

// ------------------------------------------------------------------------------------------ params
static void derive(const clrrt_params& q, DevParams& d, int n_obs) {
  memset(&d, 0, sizeof(d));
  d.dmax = q.veh.dmax; d.ddmax = q.veh.ddmax; d.Td = q.veh.Td; d.Ta = q.veh.Ta;
  d.amin = q.veh.amin; d.amax = q.veh.amax; d.L = q.veh.L; d.Vch = q.veh.Vch; d.Kus = q.veh.Kus;
  d.dt = q.sim_dt; d.tla = q.ctrl_tla; d.mindla = q.ctrl_mindla;
  d.dla_c = q.ctrl_mindla - q.ctrl_tla * q.ctrl_dlavmin;  // controller.cpp:14
  d.Kp = q.ctrl_Kp; d.Ki = q.ctrl_Ki; d.ref_res = q.ref_res; d.vmax = q.vmax; d.ay_road_max = q.ay_road_max;
  d.g0 = q.goal[0]; d.g1 = q.goal[1]; d.g2 = q.goal[2]; d.g3 = q.goal[3];
  d.W0 = q.Wcost[0]; d.W1 = q.Wcost[1]; d.W2 = q.Wcost[2]; d.W3 = q.Wcost[3]; d.W4 = q.Wcost[4];
  d.lane_shift0 = q.lane_shift0; d.Cxy1 = q.Cxy[1]; d.Cxy2 = q.Cxy[2];
  d.feas_len = 2.1 * q.ref_res;
  // getGoalReference reference.cpp:27-50 (query constants)
  double dla_end = std::max(q.ctrl_mindla, d.dla_c + q.ctrl_tla * std::abs(q.goal[3]));
  double Dext = dla_end, Dal = 1;
  const double* g = q.goal;
  double sg2, cg2;
  ::sincos(g[2], &sg2, &cg2);  // getGoalReference: cos and sin of one argument -> glibc sincos
  d.gbP1x = g[0] + Dal * cg2; d.gbP1y = g[1] + Dal * sg2;
  d.gbP2x = g[0] - Dal * cg2; d.gbP2y = g[1] - Dal * sg2;
  d.gbF1x = d.gbP1x + (Dext + Dal) * cg2; d.gbF1y = d.gbP1y + (Dext + Dal) * sg2;
  d.gbF2x = d.gbP2x + (Dext + Dal) * cg2; d.gbF2y = d.gbP2y + (Dext + Dal) * sg2;
  // feasibleGoalBias rrtplanner.cpp:294-299 (the .y coordinates use cos, as the reference does)
  double R1 = 4.77;
  d.gbR2 = R1 - 0.3;
  d.gbLx = g[0] + R1 * cos(g[2] - M_PI_2); d.gbLy = g[1] + R1 * cos(g[2] - M_PI_2);
  d.gbRx = g[0] + R1 * cos(g[2] + M_PI_2); d.gbRy = g[1] + R1 * cos(g[2] + M_PI_2);
  d.bend = q.bend; d.obs_use_pred = q.obs_use_pred; d.sort_limit = std::min(q.sort_limit, CAND_K);
  // CLRRT_COLLISION_OCC: the kernels' obstacle-list code is mode 1's; the grid test is the OCC instantiations'
  d.coll_mode = q.collision_mode == CLRRT_COLLISION_OCC ? CLRRT_COLLISION_OBB : q.collision_mode;
  int n = 0;
  while (n < (20 / q.sim_dt)) n++;  // `for(int i = 0; i<(20/sim_dt); i++)` simulation.cpp:58
  d.n_steps_max = n;
  d.use_exp = !(q.Wcost[2] == 0.0 && q.Wcost[3] >= 0.0);  // W2*exp(-W3*Dobs) is exactly +0 otherwise
  d.n_obs = n_obs;
  d.need_gap = (d.coll_mode == CLRRT_COLLISION_OBB) && d.use_exp;
}


static void bbox_reset(clrrt_ctx* c) {
  c->bbox[0] = c->bbox[1] = HUGE_VAL;
  c->bbox[2] = c->bbox[3] = -HUGE_VAL;
}
static void bbox_add(clrrt_ctx* c, double x0, double y0, double x1, double y1) {
  c->bbox[0] = std::min(c->bbox[0], x0); c->bbox[1] = std::min(c->bbox[1], y0);
  c->bbox[2] = std::max(c->bbox[2], x1); c->bbox[3] = std::max(c->bbox[3], y1);
}

// Region holding the samples (sampleAroundVehicle rrtplanner.cpp:187-201: rLong in [0, dGoal+10],
// rLat in [-7, 7] about the goal heading) and the goal, with a margin; nodes outside it go to the
// index's always-scanned overflow cell.
static void sample_region(const clrrt_params& q, double& x0, double& y0, double& x1, double& y1) {
  const double* g = q.goal;
  double dGoal = std::sqrt(g[0] * g[0] + g[1] * g[1]);
  double hd = std::atan2(g[1], g[0]);
  double ch = std::cos(hd), sh = std::sin(hd);
  x0 = y0 = 1e300; x1 = y1 = -1e300;
  for (double L : {0.0, dGoal + 10})
    for (double W : {-7.0, 7.0}) {
      double x = L * ch - W * sh, y = L * sh + W * ch;
      x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
    }
  x0 = std::min(x0, g[0]); x1 = std::max(x1, g[0]); y0 = std::min(y0, g[1]); y1 = std::max(y1, g[1]);
  const double m = 2.0;
  x0 -= m; y0 -= m; x1 += m; y1 += m;
}

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" {

int clrrt_abi_version(void) { return CLRRT_ABI_VERSION; }
static_assert(sizeof(clrrt_exchange_io) == 128, "clrrt_exchange_io layout (clrrt/abi.py ExchangeIO)");

int clrrt_params_default(clrrt_params* p, double v0, const double goal[4], double vmax) {
  if (!p) return CLRRT_EINVAL;
  memset(p, 0, sizeof(*p));
  // Vehicle::setPrius vehicle.h:39-60
  p->veh.dmax = 0.52; p->veh.ddmax = 0.3294; p->veh.Td = 0.3; p->veh.Ta = 0.3;
  p->veh.amin = -6; p->veh.amax = 2; p->veh.L = 2.7;
  double lf = 1.0868, lr = 1.6132, Cf = 22201, Cr = 22201, m = 950 + 640;
  p->veh.Kus = (m / p->veh.L) * (lr / Cf - lf / Cr);
  p->veh.Vch = 20;
  // parameters.launch:3-20
  p->ctrl_tla = 1.4; p->ctrl_mindla = 3.2; p->ctrl_dlavmin = 3; p->ref_int = 0.02; p->ref_mindist = 0.2;
  p->sim_dt = 0.04; p->ctrl_Kp = 8; p->ctrl_Ki = 0.05;
  p->Wcost[0] = 10; p->Wcost[1] = 5; p->Wcost[2] = 0; p->Wcost[3] = 4; p->Wcost[4] = 1;
  // updateReferenceResolution controller.cpp:18-21 at the query's start velocity
  p->ref_res = std::max(std::abs(v0) * p->ref_int, p->ref_mindist);
  p->vmax = vmax;
  p->ay_road_max = 0;  // rrt_node.cpp:16, never assigned
  for (int i = 0; i < 4; i++) p->goal[i] = goal ? goal[i] : 0.0;
  p->bend = 0;
  p->obs_use_pred = 1;  // rrt_node.cpp:11
  p->sort_limit = 10;   // rrtplanner.cpp:13
  p->collision_mode = CLRRT_COLLISION_STUB;
  return CLRRT_OK;
}

// glibc random_r TYPE_3 (degree 31, separation 3), seeded like srandom_r: r[0..30] = state,
// r[31] = front index, r[32] = rear index.
void clrrt_rng_seed(clrrt_rng* g, uint32_t seed) {
  int32_t* s = g->r;
  int32_t word = (int32_t)(seed == 0 ? 1 : seed);
  s[0] = word;
  for (int i = 1; i < 31; i++) {
    int32_t hi = word / 127773, lo = word % 127773;
    word = 16807 * lo - 2836 * hi;
    if (word < 0) word += 2147483647;
    s[i] = word;
  }
  s[31] = 3;
  s[32] = 0;
  s[33] = 0;
  g->pos = 0;
  for (int i = 0; i < 310; i++) clrrt_rng_next(g);
}

int32_t clrrt_rng_next(clrrt_rng* g) {
  int32_t* s = g->r;
  int f = s[31], r = s[32];
  uint32_t v = (uint32_t)s[f] + (uint32_t)s[r];
  s[f] = (int32_t)v;
  int32_t out = (int32_t)(v >> 1);
  f = f + 1 == 31 ? 0 : f + 1;
  r = r + 1 == 31 ? 0 : r + 1;
  s[31] = f;
  s[32] = r;
  return out;
}

// sampleAroundVehicle rrtplanner.cpp:187-201 (rLong, rLat) + heuristic draw :142-143 (r).
int clrrt_draw_samples(const clrrt_params* p, clrrt_rng* rng, int32_t n, clrrt_sample* out) {
  if (!p || !rng || (n > 0 && !out)) return CLRRT_EINVAL;
  const double* g = p->goal;
  const double RM = 2147483647.0;  // RAND_MAX
  double dGoal = sqrt(g[0] * g[0] + g[1] * g[1]);
  double hd = atan2(g[1], g[0]);
  double latMin = -7, latMax = 7;
  float fl = (float)(RM / (dGoal + 10));
  float fw = (float)(RM / (latMax - latMin));
  double ch, sh, cq, sq;
  ::sincos(hd, &sh, &ch);  // sampleAroundVehicle: cos/sin pairs of one argument -> glibc sincos
  ::sincos(hd + M_PI / 2, &sq, &cq);
  for (int j = 0; j < n; j++) {
    double rLong = (float)clrrt_rng_next(rng) / fl;
    double rLat = latMin + (float)clrrt_rng_next(rng) / fw;
    out[j].x = rLong * ch + rLat * cq;
    out[j].y = rLong * sh + rLat * sq;
    double r = (double)clrrt_rng_next(rng) / (double)(2147483647 / 1);
    out[j].explore = r <= ((0 * 0.3) + (1 * 0.7));  // RRT.goalReached is never set
    out[j].pad = 0;
  }
  return CLRRT_OK;
}

const char* clrrt_last_error(const clrrt_ctx* c) { return c ? c->err.c_str() : "null context"; }

// The six buffers of a list set for batches of B samples.
static int alloc_lists(clrrt_ctx* c, ListSet& s, int64_t B) {
  HIPC(c, c->mem.renew(&s.d_samples, B));
  HIPC(c, c->mem.renew_host(&s.h_samples, B));
  HIPC(c, c->mem.renew(&s.cand, B * CAND_K));
  HIPC(c, c->mem.renew(&s.ckey, B * CAND_K));
  HIPC(c, c->mem.renew(&s.ncand, B));
  HIPC(c, c->mem.renew(&s.ctie, B));
  return CLRRT_OK;
}

// Drain the streams that exist, then the memory, then the events and the streams themselves.
static void free_all(clrrt_ctx* c) {
  for (hipStream_t s : {c->side, c->side2, c->mst, c->stream})
    if (s) hipStreamSynchronize(s);
  c->mem.release_all();
  for (auto e : c->occ_ev)
    if (e) hipEventDestroy(e);
  for (auto e : c->clr_ev)
    if (e) hipEventDestroy(e);
  for (ListSet& s : c->sets)
    for (hipEvent_t e : {s.ev, s.evw, s.evm})
      if (e) hipEventDestroy(e);
  for (hipEvent_t e : {c->ev_tree, c->ev_walk, c->ev_commit})
    if (e) hipEventDestroy(e);
  for (auto& pe : c->ev_pending) { hipEventDestroy(pe.second.first); hipEventDestroy(pe.second.second); }
  for (auto e : c->ev_pool) hipEventDestroy(e);
  for (hipStream_t s : {c->side2, c->mst, c->side})
    if (s) hipStreamDestroy(s);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
}

int clrrt_create(const clrrt_params* p, const clrrt_capacity* cap, int device, clrrt_ctx** out) {
  if (!p || !out) return CLRRT_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CLRRT_EHIP;
  if (device < 0 || device >= ndev) return CLRRT_EINVAL;
  clrrt_ctx* c = new clrrt_ctx();
  c->device = device;
  c->params = *p;
  c->debug_sync = getenv("CLRRT_DEBUG_SYNC") != nullptr;
  clrrt_capacity dc;
  dc.max_nodes = 1 << 20;
  dc.max_rows = 1 << 24;
  dc.max_batch = 4096;
  dc.max_obstacles = 4096;
  c->cap = cap ? *cap : dc;
  if (c->cap.max_nodes < 2 || c->cap.max_rows < 2 || c->cap.max_batch < 1 || c->cap.max_obstacles < 0) {
    delete c;
    return CLRRT_EINVAL;
  }
  derive(c->params, c->dp, 0);
  int rc = CLRRT_OK;
  auto chk = [&](hipError_t e) {
    if (e != hipSuccess && rc == CLRRT_OK) { rc = CLRRT_EHIP; c->err = hipGetErrorString(e); }
  };
  chk(hipSetDevice(device));
  chk(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->own_stream = true;
  const int64_t B = c->cap.max_batch;
  chk(c->mem.renew(&c->tree, c->cap.max_nodes));
  chk(c->mem.renew(&c->nn, c->cap.max_nodes));
  chk(c->mem.renew(&c->arena, (size_t)c->cap.max_rows * 10));
  chk(c->mem.renew(&c->obs, std::max<int64_t>(1, c->cap.max_obstacles)));
  for (int q = 0; q < 2; q++)
    if (rc == CLRRT_OK) rc = alloc_lists(c, c->sets[q], B);
  c->partial_cap = std::max<int64_t>(B * 16, 4096) * NN_K;
  chk(c->mem.renew(&c->pk, c->partial_cap));
  chk(c->mem.renew(&c->pi, c->partial_cap));
  chk(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  chk(hipEventCreateWithFlags(&c->ev_tree, hipEventDisableTiming));
  chk(hipEventCreateWithFlags(&c->ev_walk, hipEventDisableTiming));
  chk(hipEventCreateWithFlags(&c->ev_commit, hipEventDisableTiming));
  chk(c->mem.renew(&c->res_spec, B * CAND_K));
  chk(c->mem.renew(&c->regnodes, B));
  chk(c->mem.renew(&c->res_gb, B * CAND_K));
  c->slot_rows = 0;  // slots allocated on first use (ensure_slots)
  chk(c->mem.renew_bytes(&c->rep_buf, replay_bytes() * (size_t)2 * B));
  chk(c->mem.renew(&c->gbnodes, B));
  chk(c->mem.renew(&c->so, B));
  chk(c->mem.renew(&c->first_conflict, 1));
  chk(c->mem.renew(&c->out_nodes, 2 * B));
  chk(c->mem.renew(&c->jobs, 2 * B));
  chk(c->mem.renew(&c->totals, 8));
  chk(c->mem.renew(&c->cmp.packed, B));
  chk(c->mem.renew(&c->cmp.scanned, B));
  c->cmp.tmp_bytes = compact_scan_bytes((int)B);
  chk(c->mem.renew_bytes(&c->cmp.tmp, std::max<size_t>(c->cmp.tmp_bytes, 256)));
  chk(c->mem.renew(&c->nn_seed, B));
  chk(c->mem.renew(&c->roll_q, 1));
  chk(c->mem.renew(&c->roll_best, B));
  chk(c->mem.renew(&c->roll_perm, (int64_t)B * CAND_K));
  chk(c->mem.renew(&c->roll_pflag, (int64_t)roll_order_ints((int)(B * CAND_K))));
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
      c->n_cu = ncu;
  }
  chk(c->mem.renew(&c->d_bbox, 4));
  chk(c->mem.renew_host(&c->h_bbox, 4));
  chk(c->mem.renew(&c->work_ctr, 64));
  if (rc == CLRRT_OK) chk(hipMemset(c->work_ctr, 0, 64 * sizeof(unsigned long long)));
  chk(c->mem.renew_host(&c->h_totals, 8));
  chk(c->mem.renew_host(&c->h_int, 4));
  if (rc != CLRRT_OK) {
    fprintf(stderr, "clrrt_create: %s\n", c->err.c_str());
    free_all(c);
    delete c;
    return rc;
  }
  *out = c;
  return CLRRT_OK;
}

void clrrt_destroy(clrrt_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  free_all(c);
  delete c;
}

int clrrt_set_stream(clrrt_ctx* c, void* s) {
  if (!c) return CLRRT_EINVAL;
  HIPC(c, hipStreamSynchronize(c->stream));
  if (c->own_stream) hipStreamDestroy(c->stream);
  if (s) {
    c->stream = (hipStream_t)s;
    c->own_stream = false;
  } else {
    HIPC(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return CLRRT_OK;
}

int clrrt_set_rank(clrrt_ctx* c, int32_t rank) {
  if (!c || rank < 0) return CLRRT_EINVAL;
  c->rank = rank;
  return CLRRT_OK;
}

int clrrt_set_params(clrrt_ctx* c, const clrrt_params* p) {
  if (!c || !p) return CLRRT_EINVAL;
  pf_reset(c);
  DevParams d;
  derive(*p, d, c->n_obs);
  int rc = flush_replays(c);  // pending replays run under the parameters they were committed with
  if (rc != CLRRT_OK) return rc;
  if (c->slots && d.n_steps_max + 1 > c->slot_rows) {  // a smaller sim_dt needs longer rollout slots
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->slot_rows = 0;
    HIPC(c, c->mem.renew(&c->slots, (size_t)2 * (d.n_steps_max + 1) * 10 * c->cap.max_batch * CAND_K));
    c->slot_rows = d.n_steps_max + 1;
  }
  c->params = *p;
  c->dp = d;
  return CLRRT_OK;
}

}  // extern "C"

// Uniform grid over the static obstacles for the rollout's collision cull (see ObsGrid).  The
// cell size starts near 1/1024 of the covered area and grows until the grid fits the LDS budget.
static const float kVehRad = 2.6220219f, kCullMargin = 0.05f;  // = VEH_RAD, CULL_MARGIN (kernels)
static int build_grid(clrrt_ctx* c, const std::vector<BakedObs>& b) {
  // `mov`: the obstacles tested at every step, ascending -- the moving ones and those exempt from culling
  std::vector<int> stat, mov;
  c->grid_exempt = 0;
  for (int i = 0; i < (int)b.size(); i++) {
    const bool exempt = std::isinf(b[i].brad);
    c->grid_exempt += exempt;
    (b[i].moving || exempt ? mov : stat).push_back(i);
  }
  const double tol = 0.05;
  double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
  std::vector<double> rr(b.size());
  for (int i : stat) {
    rr[i] = (double)(b[i].brad + kVehRad + kCullMargin);
    double cx = (double)(float)b[i].cx, cy = (double)(float)b[i].cy;
    x0 = std::min(x0, cx - rr[i] - tol); x1 = std::max(x1, cx + rr[i] + tol);
    y0 = std::min(y0, cy - rr[i] - tol); y1 = std::max(y1, cy + rr[i] + tol);
  }
  std::vector<uint32_t> start;
  std::vector<uint16_t> items;
  int gw = 0, gh = 0;
  float fx0 = 0, fy0 = 0, finv = 0;
  // dynamic LDS of the rollout kernels (36 B per obstacle + grid): the rollout kernels run one
  // 256-lane block per CU (256 VGPRs), so up to ~140 KiB of the CU's 160 KiB serve the grid
  // (launches raise hipFuncAttributeMaxDynamicSharedMemorySize accordingly)
#ifndef CLRRT_OBS_LDS_KB
#define CLRRT_OBS_LDS_KB 120
#endif
  const size_t lds_cap = CLRRT_OBS_LDS_KB * 1024;
  const size_t per_obs = 6 * 16 + 4;  // kernel LDS per obstacle: cull table + SAT geometry (roll_lds_bytes)
  const size_t lds_budget = b.size() * per_obs < lds_cap ? lds_cap - b.size() * per_obs : 0;
  if (!stat.empty() && std::isfinite(x0) && std::isfinite(x1) && std::isfinite(y0) && std::isfinite(y1) &&
      lds_budget >= 4 * 1024) {
    double W = x1 - x0, H = y1 - y0;
    double cs = std::max(0.25, std::sqrt(W * H / 8192.0));
    for (int attempt = 0; attempt < 40; attempt++, cs *= 1.25) {
      finv = (float)(1.0 / cs);
      fx0 = (float)x0; fy0 = (float)y0;
      // effective cell size seen by the kernel's float arithmetic
      double ecs = 1.0 / (double)finv;
      gw = (int)std::ceil((x1 - fx0) / ecs) + 1;
      gh = (int)std::ceil((y1 - fy0) / ecs) + 1;
      if ((int64_t)gw * gh > 16384) continue;
      start.assign((size_t)gw * gh + 1, 0);
      items.clear();
      for (int gy = 0; gy < gh; gy++)
        for (int gx = 0; gx < gw; gx++) {
          start[(size_t)gy * gw + gx] = (uint32_t)items.size();
          double rx0 = fx0 + gx * ecs - tol, rx1 = fx0 + (gx + 1) * ecs + tol;
          double ry0 = fy0 + gy * ecs - tol, ry1 = fy0 + (gy + 1) * ecs + tol;
          for (int i : stat) {
            double cx = (double)(float)b[i].cx, cy = (double)(float)b[i].cy;
            double dx = std::max(0.0, std::max(rx0 - cx, cx - rx1));
            double dy = std::max(0.0, std::max(ry0 - cy, cy - ry1));
            if (dx * dx + dy * dy > (rr[i] + tol) * (rr[i] + tol)) continue;
            // the kernel's second cull: the vehicle circle (VEH_RAD + margin) against the obstacle box.
            // A separating-axis gap between the cell and the (slackened) box bounds their distance from
            // below, so a gap beyond the circle radius proves no centre in the cell survives that cull.
            const double P = b[i].P, Q = b[i].Q, R = b[i].R, S = b[i].S;
            const double hh = std::sqrt(P * P + R * R), ww = std::sqrt(Q * Q + S * S);
            const double ux = hh > 0 ? P / hh : 1.0, uy = hh > 0 ? R / hh : 0.0;
            const double eh = hh * 1.0001 + 1e-3, ew = ww * 1.0001 + 1e-3;
            const double rcx = 0.5 * (rx0 + rx1), rcy = 0.5 * (ry0 + ry1);
            const double hx = 0.5 * (rx1 - rx0), hy = 0.5 * (ry1 - ry0);
            const double ex = std::fabs(ux) * eh + std::fabs(uy) * ew, ey = std::fabs(uy) * eh + std::fabs(ux) * ew;
            double gap = std::max(std::fabs(cx - rcx) - hx - ex, std::fabs(cy - rcy) - hy - ey);
            const double du = (cx - rcx) * ux + (cy - rcy) * uy, dv = -(cx - rcx) * uy + (cy - rcy) * ux;
            gap = std::max(gap, std::fabs(du) - eh - (hx * std::fabs(ux) + hy * std::fabs(uy)));
            gap = std::max(gap, std::fabs(dv) - ew - (hx * std::fabs(uy) + hy * std::fabs(ux)));
            if (gap > (double)(kVehRad + kCullMargin) + tol) continue;
            items.push_back((uint16_t)i);
          }
        }
      start[(size_t)gw * gh] = (uint32_t)items.size();
      size_t bytes = 4 * start.size() + 2 * (items.size() + mov.size());
      if (bytes <= lds_budget) break;
      gw = gh = 0;
    }
  }
  if (gw == 0) { start.clear(); items.clear(); }
  size_t need = 4 * start.size() + 2 * (items.size() + mov.size()) + 16;
  if (need > c->grid_bytes) {
    c->grid_bytes = 0;
    HIPC(c, c->mem.renew_bytes(&c->grid_buf, need));
    c->grid_bytes = need;
  }
  std::vector<uint8_t> host(need, 0);
  size_t o_items = 4 * start.size(), o_mov = o_items + 2 * items.size();
  if (!start.empty()) memcpy(host.data(), start.data(), 4 * start.size());
  if (!items.empty()) memcpy(host.data() + o_items, items.data(), 2 * items.size());
  for (size_t k = 0; k < mov.size(); k++) {
    uint16_t v = (uint16_t)mov[k];
    memcpy(host.data() + o_mov + 2 * k, &v, 2);
  }
  HIPC(c, hipMemcpyAsync(c->grid_buf, host.data(), need, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  ObsGrid& g = c->grid;
  g.start = (const uint32_t*)c->grid_buf;
  g.items = (const uint16_t*)((const uint8_t*)c->grid_buf + o_items);
  g.mov = (const uint16_t*)((const uint8_t*)c->grid_buf + o_mov);
  g.gw = gw; g.gh = gh;
  g.nitems = (int)items.size();
  g.nmov = (int)mov.size();
  g.x0 = fx0; g.y0 = fy0; g.inv = finv;
  return CLRRT_OK;
}

// getOBBvector old_collisioncheck.cpp:14-16 + OBB::setVertices/setNorms :56-76 for one obstacle, hoisted
// out of the step loop: the float products (P, Q, R, S) always, the float SAT geometry of a static one.
static void bake_obstacle(const clrrt_obstacle& o, BakedObs& d) {
  memset(&d, 0, sizeof(d));
  float w = (float)(o.size_x / 2), h = (float)(o.size_y / 2), th = (float)o.theta;
  float cf, sf;
  ::sincosf(th, &sf, &cf);  // OBB::setVertices: float cos/sin of one argument -> glibc sincosf
  float hh = h / 2, ww = w / 2;
  d.P = cf * hh; d.Q = sf * ww; d.R = sf * hh; d.S = cf * ww;
  d.cx = o.cx; d.cy = o.cy; d.vlx = o.vx; d.vly = o.vy;
  d.moving = (o.vx != 0.0 || o.vy != 0.0);
  // static geometry: centre + 0*t (t >= 0) == centre + 0.0
  double px = o.cx + 0.0, py = o.cy + 0.0;
  d.vx[0] = (float)((px + (double)d.P) - (double)d.Q);
  d.vy[0] = (float)((py + (double)d.R) + (double)d.S);
  d.vx[1] = (float)((px + (double)d.P) - (double)(-d.Q));
  d.vy[1] = (float)((py + (double)d.R) + (double)(-d.S));
  d.vx[2] = (float)((px + (double)(-d.P)) - (double)(-d.Q));
  d.vy[2] = (float)((py + (double)(-d.R)) + (double)(-d.S));
  d.vx[3] = (float)((px + (double)(-d.P)) - (double)d.Q);
  d.vy[3] = (float)((py + (double)(-d.R)) + (double)d.S);
  for (int k = 0; k < 3; k++) {
    d.nx[k] = d.vy[k + 1] - d.vy[k];
    d.ny[k] = -(d.vx[k + 1] - d.vx[k]);
  }
  d.nx[3] = d.vy[0] - d.vy[3];
  d.ny[3] = -(d.vx[0] - d.vx[3]);
  d.bcx = (float)o.cx; d.bcy = (float)o.cy;
  d.brad = std::sqrt(hh * hh + ww * ww);
}

extern "C" {

// getOBBvector old_collisioncheck.cpp:6-22, evaluated once per query instead of once per step.
int clrrt_set_obstacles(clrrt_ctx* c, const clrrt_obstacle* o, int32_t m) {
  if (!c || m < 0 || (m > 0 && !o)) return CLRRT_EINVAL;
  if (m > c->cap.max_obstacles) return fail(c, CLRRT_ECAPACITY, "too many obstacles");
  if (m > 1400) return fail(c, CLRRT_ECAPACITY, "at most 1400 obstacles (rollout LDS cull table)");
  std::vector<BakedObs> b(m);
  for (int i = 0; i < m; i++) {
    bake_obstacle(o[i], b[i]);
    // beyond CULL_EXEMPT_BOUND the culls' margin no longer covers the float rounding of the reference's SAT: such an
    // obstacle is never culled (a non-finite one neither)
    const double reach = std::max(std::fabs(o[i].cx) + std::fabs(o[i].vx) * CULL_EXEMPT_HORIZON,
                                  std::fabs(o[i].cy) + std::fabs(o[i].vy) * CULL_EXEMPT_HORIZON) +
                         (double)b[i].brad + 16.0;
    if (!(reach < CULL_EXEMPT_BOUND)) b[i].brad = INFINITY;
  }
  HIPC(c, hipSetDevice(c->device));
  int frc = flush_replays(c);  // pending replays collide against the obstacles they were committed with
  if (frc != CLRRT_OK) return frc;
  if (m > 0) {
    HIPC(c, hipMemcpyAsync(c->obs, b.data(), sizeof(BakedObs) * m, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
  }
  c->n_obs = m;
  derive(c->params, c->dp, m);
  return build_grid(c, b);
}

// The distance field of the grid in c->occ (set, clearance on), baked on the context's stream, which the caller has
// drained of launches that read the old field; on success c->occ carries it.
static int bake_field(clrrt_ctx* c) {
  OccGrid& g = c->occ;
  g.field = nullptr;
  g.clear_max = 0.0;
  c->clr_bake_ms = 0.f;
  const size_t ncell = (size_t)g.w * g.h * g.layers;  // (layer k's field: w h dwords behind layer k - 1's)
  const size_t field_b = (sizeof(uint32_t) * ncell + 255) / 256 * 256, rowd_b = (sizeof(uint16_t) * ncell + 255) / 256 * 256;
  const size_t need = field_b + rowd_b + 64 * sizeof(uint32_t) * g.layers;
  if (need > c->clr_bytes) {
    c->clr_bytes = 0;
    HIPC(c, c->mem.renew_bytes(&c->clr_buf, need));
    c->clr_bytes = need;
  }
  for (auto& e : c->clr_ev)
    if (!e) HIPC(c, hipEventCreate(&e));
  char* b = (char*)c->clr_buf;
  HIPC(c, hipEventRecord(c->clr_ev[0], c->stream));
  HIPC(c, launch_occ_field(c->stream, g, (uint16_t*)(b + field_b), (uint32_t*)(b + field_b + rowd_b), (uint32_t*)b));
  HIPC(c, hipEventRecord(c->clr_ev[1], c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, hipEventElapsedTime(&c->clr_bake_ms, c->clr_ev[0], c->clr_ev[1]));
  g.field = (const uint32_t*)b;
  g.field_stride = g.w * g.h;
  g.clear_max = c->clr_max;
  return CLRRT_OK;
}

// clrrt_set_occupancy (one layer) and clrrt_set_occupancy_layers: `fn` names the call in the error texts.
static int set_occ_stack(clrrt_ctx* c, const clrrt_occupancy* o, int32_t layers, double t0, double dt,
                         const uint8_t* cells, const std::string& fn) {
  if (!c) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (!o || o->w == 0) {  // clear
    const int frc = flush_replays(c);  // pending replays collide against the scene they were committed with
    if (frc != CLRRT_OK) return frc;
    c->occ = OccGrid{};
    c->occ_count = 0;
    for (auto& n : c->occ_counts) n = 0;
    c->occ_bake_ms = 0.f;
    return CLRRT_OK;
  }
  if (layers < 1 || layers > CLRRT_OCC_MAX_LAYERS)
    return fail(c, CLRRT_EINVAL, fn + ": layers outside [1, " + std::to_string(CLRRT_OCC_MAX_LAYERS) + "]");
  if (o->w < 0 || o->w > 2048) return fail(c, CLRRT_EINVAL, fn + ": w outside [0, 2048]");
  if (o->h < 1 || o->h > 2048) return fail(c, CLRRT_EINVAL, fn + ": h outside [1, 2048]");
  if ((int64_t)o->w * o->h > ((int64_t)1 << 22)) return fail(c, CLRRT_EINVAL, fn + ": w * h above 2^22");
  if ((int64_t)o->w * o->h * layers > ((int64_t)1 << 24))
    return fail(c, CLRRT_EINVAL, fn + ": w * h * layers above 2^24");
  if (!std::isfinite(t0)) return fail(c, CLRRT_EINVAL, fn + ": t0 is not finite");
  if (!(std::isfinite(dt) && dt > 0.0)) return fail(c, CLRRT_EINVAL, fn + ": dt is not finite and > 0");
  if (!std::isfinite(o->x0)) return fail(c, CLRRT_EINVAL, fn + ": x0 is not finite");
  if (!std::isfinite(o->y0)) return fail(c, CLRRT_EINVAL, fn + ": y0 is not finite");
  if (!(std::isfinite(o->res) && o->res > 0.0)) return fail(c, CLRRT_EINVAL, fn + ": res is not finite and > 0");
  if (!(std::isfinite(o->inflate) && o->inflate >= 0.0 && o->inflate <= 1000.0))
    return fail(c, CLRRT_EINVAL, fn + ": inflate is not finite and within [0, 1000]");
  if (!cells) return fail(c, CLRRT_EINVAL, fn + ": cells is NULL");
  // the reach map (clrrt_occ.hpp): cells of rk x rk occupancy cells, about max(0.5 m, R / 8) wide, rm of them around
  // the grid; Rc: the reach radius plus the rounding slack, in occupancy cells
  const double R = std::sqrt(2.424 * 2.424 + 1.0) + o->inflate * std::sqrt(2.0);
  const double ext = std::max(o->w, o->h) * o->res + 2.0 * R;
  const double mag = std::fabs(o->x0) + std::fabs(o->y0) + ext;
  if (!(o->res >= mag * (1.0 / 1073741824.0)))
    return fail(c, CLRRT_EINVAL, fn + ": res is below 2^-30 of the grid's coordinates");
  OccGrid g{};
  g.x0 = o->x0; g.y0 = o->y0; g.res = o->res; g.inflate = o->inflate;
  g.w = o->w; g.h = o->h;
  g.ws = 2 * ((o->w + 63) / 64);
  g.rk = std::max(1, (int)std::floor(std::max(0.5, R / 8.0) / o->res + 0.5));
  const double Rc = (R + o->res / 64.0 + 1e-9 * mag) / o->res;
  g.rm = (int)std::ceil(Rc / g.rk) + 1;
  g.rw = (o->w + g.rk - 1) / g.rk + 2 * g.rm;
  g.rh = (o->h + g.rk - 1) / g.rk + 2 * g.rm;
  g.rws = 2 * ((g.rw + 63) / 64);
  g.rres = g.rk * o->res;
  g.rx0 = o->x0 - g.rm * g.rres;
  g.ry0 = o->y0 - g.rm * g.rres;
  g.layers = layers;
  g.t0 = t0; g.dt = dt;
  g.occ_stride = g.h * g.ws;
  g.reach_stride = g.rh * g.rws;
  const size_t ncell = (size_t)o->w * o->h * layers;
  const size_t cell_b = (ncell + 255) / 256 * 256;
  const size_t occ_b = sizeof(uint32_t) * (size_t)g.occ_stride * layers;
  const size_t reach_b = sizeof(uint32_t) * (size_t)g.reach_stride * layers;
  const size_t union_b = layers > 1 ? sizeof(uint32_t) * (size_t)g.reach_stride : 0;
  const size_t need = cell_b + 256 + occ_b + reach_b + union_b;
  const int frc = flush_replays(c);  // pending replays collide against the scene they were committed with
  if (frc != CLRRT_OK) return frc;
  HIPC(c, hipStreamSynchronize(c->stream));  // (no launch still reads the old maps)
  if (need > c->occ_bytes) {
    c->occ_bytes = 0;
    c->occ = OccGrid{};
    HIPC(c, c->mem.renew_bytes(&c->occ_buf, need));
    c->occ_bytes = need;
  }
  for (auto& e : c->occ_ev)
    if (!e) HIPC(c, hipEventCreate(&e));
  uint8_t* d_cells = (uint8_t*)c->occ_buf;
  unsigned int* d_count = (unsigned int*)(d_cells + cell_b);
  g.occ = (const uint32_t*)(d_cells + cell_b + 256);
  g.reach = (const uint32_t*)(d_cells + cell_b + 256 + occ_b);
  g.reach_u = layers > 1 ? (const uint32_t*)(d_cells + cell_b + 256 + occ_b + reach_b) : g.reach;
  c->occ = OccGrid{};  // (a failure below leaves no grid)
  unsigned int count[CLRRT_OCC_MAX_LAYERS] = {};
  HIPC(c, hipEventRecord(c->occ_ev[0], c->stream));
  HIPC(c, hipMemcpyAsync(d_cells, cells, ncell, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemsetAsync(d_count, 0, sizeof(count), c->stream));
  HIPC(c, launch_occ_bake(c->stream, d_cells, g, Rc, d_count));
  HIPC(c, hipEventRecord(c->occ_ev[1], c->stream));
  HIPC(c, hipMemcpyAsync(count, d_count, sizeof(count), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, hipEventElapsedTime(&c->occ_bake_ms, c->occ_ev[0], c->occ_ev[1]));
  c->occ = g;
  c->occ_count = 0;
  for (int k = 0; k < CLRRT_OCC_MAX_LAYERS; k++) c->occ_count += c->occ_counts[k] = count[k];
  if (c->clr_max > 0.0) return bake_field(c);
  return CLRRT_OK;
}

int clrrt_set_occupancy(clrrt_ctx* c, const clrrt_occupancy* o, const uint8_t* cells) {
  return set_occ_stack(c, o, 1, 0.0, 1.0, cells, "set_occupancy");
}

int clrrt_set_occupancy_layers(clrrt_ctx* c, const clrrt_occupancy* o, int32_t layers, double t0, double dt,
                               const uint8_t* cells) {
  return set_occ_stack(c, o, layers, t0, dt, cells, "set_occupancy_layers");
}


int clrrt_set_occupancy_clearance(clrrt_ctx* c, double clear_max) {
  if (!c) return CLRRT_EINVAL;
  if (!(clear_max >= 0.0 && std::isfinite(clear_max)))
    return fail(c, CLRRT_EINVAL, "set_occupancy_clearance: clear_max = " + std::to_string(clear_max) +
                                     " is not 0 (off) or finite and > 0");
  HIPC(c, hipSetDevice(c->device));
  const int frc = flush_replays(c);  // pending replays are costed as the scene they were committed with
  if (frc != CLRRT_OK) return frc;
  HIPC(c, hipStreamSynchronize(c->stream));  // (no launch still reads the old field)
  c->clr_max = clear_max;
  if (clear_max == 0.0) {
    c->occ.field = nullptr;
    c->occ.clear_max = 0.0;
    c->clr_bake_ms = 0.f;
    c->clr_bytes = 0;
    HIPC(c, c->mem.release(&c->clr_buf));
    return CLRRT_OK;
  }
  if (c->occ.w > 0) return bake_field(c);
  return CLRRT_OK;
}

int clrrt_occupancy_clearance_info(clrrt_ctx* c, clrrt_clearance_info_t* out) {
  if (!c || !out) return CLRRT_EINVAL;
  memset(out, 0, sizeof(*out));
  out->clear_max = c->clr_max;
  out->on = c->clr_max > 0.0;
  out->baked = c->occ.field != nullptr;
  out->field_bytes = out->baked ? (int64_t)sizeof(uint32_t) * c->occ.w * c->occ.h * c->occ.layers : 0;
  out->bake_ms = c->clr_bake_ms;
  return CLRRT_OK;
}

int clrrt_occupancy_field_layer(clrrt_ctx* c, int32_t layer, uint32_t* out) {
  if (!c || !out) return CLRRT_EINVAL;
  if (!c->occ.field) return fail(c, CLRRT_ESTATE, "occupancy_field: no field is baked (clrrt_set_occupancy_clearance with a grid set)");
  if (layer < 0 || layer >= c->occ.layers)
    return fail(c, CLRRT_EINVAL, "occupancy_field_layer: layer outside [0, " + std::to_string(c->occ.layers) + ")");
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(out, c->occ.field + (size_t)layer * c->occ.field_stride,
                         sizeof(uint32_t) * (size_t)c->occ.w * c->occ.h, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_occupancy_field(clrrt_ctx* c, uint32_t* out) { return clrrt_occupancy_field_layer(c, 0, out); }

int clrrt_occupancy_clearance(clrrt_ctx* c, const double* states, int32_t n, double* out) {
  if (!c || n < 0 || (n > 0 && (!states || !out))) return CLRRT_EINVAL;
  if (!c->occ.field) return fail(c, CLRRT_ESTATE, "occupancy_clearance: no field is baked (clrrt_set_occupancy_clearance with a grid set)");
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const char* const pre = "occupancy_clearance: ";
  Scratch<double> din, dout;
  HIPP(c, pre, din.alloc(10 * (size_t)n));
  HIPP(c, pre, dout.alloc(n));
  HIPP(c, pre, hipMemcpyAsync(din, states, sizeof(double) * 10 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, launch_occ_clearance(c->stream, c->occ, c->params.obs_use_pred, din, n, dout));
  HIPP(c, pre, hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

// CLRRT_OCC_* of a k_roll_run launch of `a` (the grid in a.occ).
static int occ_placement(const RollArgs& a) {
  switch (roll_occ_placement(a)) {
    case OCC_IN_LDS: return CLRRT_OCC_LDS;
    case OCC_IN_LDS_UNION: return CLRRT_OCC_REACH_LDS;
    default: return CLRRT_OCC_GLOBAL;
  }
}

int clrrt_occupancy_info(clrrt_ctx* c, clrrt_occupancy_info_t* out) {
  if (!c || !out) return CLRRT_EINVAL;
  memset(out, 0, sizeof(*out));
  const OccGrid& g = c->occ;
  if (g.w <= 0) return CLRRT_OK;
  out->w = g.w; out->h = g.h;
  out->reach_w = g.rw; out->reach_h = g.rh; out->reach_k = g.rk;
  RollArgs a = roll_args(c, 0);
  a.occ = g;  // (the placement a mode-2 launch takes, whichever mode is set now)
  a.coop_enable = c->roll_coop;
  out->placement = occ_placement(a);
  out->occupied = c->occ_count;
  out->map_bytes = (int64_t)occ_map_bytes(g);
  out->bake_ms = c->occ_bake_ms;
  return CLRRT_OK;
}

int clrrt_occupancy_layers_info(clrrt_ctx* c, clrrt_occupancy_layers_info_t* out) {
  if (!c || !out) return CLRRT_EINVAL;
  memset(out, 0, sizeof(*out));
  const OccGrid& g = c->occ;
  if (g.w <= 0) return CLRRT_OK;
  RollArgs a = roll_args(c, 0);
  a.occ = g;
  a.coop_enable = c->roll_coop;
  out->layers = g.layers;
  out->placement = occ_placement(a);
  out->t0 = g.t0;
  out->dt = g.dt;
  for (int k = 0; k < CLRRT_OCC_MAX_LAYERS; k++) out->occupied[k] = c->occ_counts[k];
  out->map_bytes = (int64_t)occ_map_bytes(g);
  out->union_reach_bytes = g.layers > 1 ? (int64_t)occ_union_bytes(g) : 0;
  out->field_bytes = g.field ? (int64_t)sizeof(uint32_t) * g.w * g.h * g.layers : 0;
  out->bake_ms = c->occ_bake_ms;
  return CLRRT_OK;
}

int clrrt_tree_init(clrrt_ctx* c, const double root_state[10]) {
  if (!c || !root_state) return CLRRT_EINVAL;
  pf_reset(c);
  c->rep_n = 0;  // replays pending for the old tree's rows: the tree is replaced
  HIPC(c, hipSetDevice(c->device));
  Scratch<double> d_state;
  HIPC(c, d_state.alloc(10));  // (HIPC, not HIPP: this failure never carried the prefix)
  HIPP(c, "tree_init: ", hipMemcpyAsync(d_state, root_state, 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPP(c, "tree_init: ", launch_init_root(c->stream, d_state, c->tree, c->nn, c->arena));
  HIPP(c, "tree_init: ", hipStreamSynchronize(c->stream));
  c->n_nodes = 1;
  c->n_rows = 1;
  c->tree_rowless = false;
  bbox_reset(c);
  if (std::isfinite(root_state[0]) && std::isfinite(root_state[1]))
    bbox_add(c, root_state[0], root_state[1], root_state[0], root_state[1]);
  return CLRRT_OK;
}

int clrrt_tree_load(clrrt_ctx* c, const clrrt_node* nodes, int64_t n) {
  if (!c || n < 0 || (n > 0 && !nodes)) return CLRRT_EINVAL;
  pf_reset(c);
  c->rep_n = 0;  // the tree is replaced
  if (n > c->cap.max_nodes) return fail(c, CLRRT_ECAPACITY, "tree_load: too many nodes");
  HIPC(c, hipSetDevice(c->device));
  if (n > 0) {
    Scratch<clrrt_node> tmp;
    HIPC(c, tmp.alloc(n));  // (HIPC, not HIPP: this failure never carried the prefix)
    HIPP(c, "tree_load: ", hipMemcpyAsync(tmp, nodes, sizeof(clrrt_node) * n, hipMemcpyHostToDevice, c->stream));
    HIPP(c, "tree_load: ", launch_append(c->stream, tmp, (int)n, 0, c->tree, c->nn));
    HIPP(c, "tree_load: ", hipStreamSynchronize(c->stream));
  }
  c->n_nodes = n;
  c->n_rows = 0;
  c->tree_rowless = true;
  bbox_reset(c);
  for (int64_t i = 0; i < n; i++)
    if (std::isfinite(nodes[i].state[0]) && std::isfinite(nodes[i].state[1]))
      bbox_add(c, nodes[i].state[0], nodes[i].state[1], nodes[i].state[0], nodes[i].state[1]);
  return CLRRT_OK;
}

int clrrt_tree_truncate(clrrt_ctx* c, int64_t n) {
  if (!c || n < 1 || n > c->n_nodes) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  int rc = flush_replays(c);  // pending rows of committed nodes land first (the arena stays consistent)
  if (rc != CLRRT_OK) return rc;
  pf_reset(c);  // prefetched lists and kept walk sort results describe the longer tree
  if (n == c->n_nodes) return CLRRT_OK;
  clrrt_node h;
  HIPC(c, hipMemcpyAsync(&h, c->tree + n, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  c->n_nodes = n;
  if (h.row_offset >= 0 && h.row_offset <= c->n_rows) c->n_rows = h.row_offset;  // rows are appended in node order
  return CLRRT_OK;  // (the tree's box stays a superset: a valid search frame)
}

int clrrt_tree_rebase(clrrt_ctx* c, int64_t root_id, const double pose[3], double t_shift, clrrt_rebase_info* out) {
  if (!c || !pose) return CLRRT_EINVAL;
  if (root_id < 0 || root_id >= c->n_nodes) return fail(c, CLRRT_EINVAL, "tree_rebase: root_id outside the tree");
  if (!(std::isfinite(pose[0]) && std::isfinite(pose[1]) && std::isfinite(pose[2]) && std::isfinite(t_shift)))
    return fail(c, CLRRT_EINVAL, "tree_rebase: non-finite pose or t_shift");
  if (c->sh.world > 1) return fail(c, CLRRT_ESTATE, "tree_rebase: not with a sharded tree (clrrt_set_shards world > 1)");
  if (c->tree_rowless || c->n_rows <= 0)
    return fail(c, CLRRT_ESTATE, "tree_rebase: the tree has no rows (clrrt_tree_load)");
  HIPC(c, hipSetDevice(c->device));
  int rc = flush_replays(c);  // deferred rows of committed nodes land first
  if (rc != CLRRT_OK) return rc;
  const char* const pre = "tree_rebase: ";
  const int n = (int)c->n_nodes, root = (int)root_id;
  const int64_t n_rows = c->n_rows;
  const int ts = c->dp.bend ? 2 : 1;
  hipStream_t st = c->stream;
  hipEvent_t ev0 = ev_get(c), ev1 = ev_get(c);
  if (!ev0 || !ev1) return fail(c, CLRRT_EHIP, "tree_rebase: no event");
  struct EvBack {  // the events return to the pool on every exit
    clrrt_ctx* c; hipEvent_t a, b;
    ~EvBack() { c->ev_pool.push_back(a); c->ev_pool.push_back(b); }
  } evback{c, ev0, ev1};
  // per-node scratch (ints: jump, hop, bad double-buffered, row counts, flags, one error word, one moved word), the
  // scan's buffers and the per-row cost terms (8 or 16 bytes per row of the tree: the one buffer that grows with the
  // rows; the move's window below does not)
  Scratch<int> ints;
  Scratch<int64_t> roff;
  Scratch<uint64_t> scan;
  Scratch<unsigned long long> stats;
  Scratch<double> terms, bbox;
  Scratch<char> tmp;
  const size_t tmp_bytes = compact_scan_bytes(n);
  HIPP(c, pre, ints.alloc(8 * (size_t)n + 2));
  HIPP(c, pre, roff.alloc(n));
  HIPP(c, pre, scan.alloc(2 * (size_t)n));
  HIPP(c, pre, stats.alloc(3));
  HIPP(c, pre, terms.alloc((size_t)ts * n_rows));
  HIPP(c, pre, bbox.alloc(4));
  HIPP(c, pre, tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
  int* jump[2] = {ints, ints + n};
  int* hop[2] = {ints + 2 * (size_t)n, ints + 3 * (size_t)n};
  int* bad[2] = {ints + 4 * (size_t)n, ints + 5 * (size_t)n};
  int* nrw = ints + 6 * (size_t)n;
  int* nflag = ints + 7 * (size_t)n;
  int* err = ints + 8 * (size_t)n;
  int* moved = err + 1;
  uint64_t* packed = scan;
  uint64_t* scanned = scan + n;
  HIPP(c, pre, hipEventRecord(ev0, st));
  HIPP(c, pre, hipMemsetAsync(nflag, 0, sizeof(int) * ((size_t)n + 2), st));  // flags, err, moved
  HIPP(c, pre, hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 3, st));
  HIPP(c, pre, launch_rebase_prep(st, c->tree, n, n_rows, root, roff, nrw, jump[0], hop[0], err));
  RebaseCheck ck;
  memset(&ck, 0, sizeof(ck));
  ck.a = roll_args(c, 0);
  ck.a.ctr = nullptr;
  ck.n = n; ck.root = root; ck.n_rows = n_rows;
  ck.P0 = pose[0]; ck.P1 = pose[1]; ck.P2 = pose[2]; ck.t_shift = t_shift;
  ck.roff = roff; ck.nrw = nrw; ck.nflag = nflag; ck.terms = terms; ck.tstride = ts;
  int h_err = 0;
  HIPP(c, pre, hipMemcpyAsync(&h_err, err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipStreamSynchronize(st));
  if (h_err != 0)  // (before the check kernel, whose row search relies on the layout)
    return fail(c, CLRRT_ESTATE, h_err == 1 ? "tree_rebase: a parent does not precede its child"
                                            : "tree_rebase: node rows are not laid out in node order");
  {
    KTimer kt(c, 6);
    HIPP(c, pre, launch_rebase_check(st, ck));
  }
  // closure and depth: passes until one moves nothing
  int cur = 0, passes = 0;
  for (bool first = true;; first = false) {
    int h_moved = 0;
    HIPP(c, pre, hipMemsetAsync(moved, 0, sizeof(int), st));
    HIPP(c, pre, launch_rebase_double(st, n, root, jump[cur], hop[cur], first ? nflag : bad[cur], jump[cur ^ 1],
                                      hop[cur ^ 1], bad[cur ^ 1], moved));
    HIPP(c, pre, hipMemcpyAsync(&h_moved, moved, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPP(c, pre, hipStreamSynchronize(st));
    cur ^= 1;
    passes++;
    if (!h_moved) break;
    if (passes > 40) return fail(c, CLRRT_ESTATE, "tree_rebase: the parent chains do not end");
  }
  HIPP(c, pre, launch_rebase_mark(st, n, root, jump[cur], hop[cur], bad[cur], nflag, nrw, packed, scanned, stats, tmp,
                                  tmp_bytes));
  unsigned long long h_stats[3];
  uint64_t h_last[2];
  int h_rootflag = 0;
  HIPP(c, pre, hipMemcpyAsync(h_stats, stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipMemcpyAsync(&h_last[0], packed + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipMemcpyAsync(&h_last[1], scanned + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipMemcpyAsync(&h_rootflag, nflag + root, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipStreamSynchronize(st));
  clrrt_rebase_info info;
  memset(&info, 0, sizeof(info));
  info.nodes_before = n;
  info.rows_before = n_rows;
  info.nodes_subtree = (int64_t)h_stats[0];
  info.nodes_collided = (int64_t)h_stats[1];
  float ms = 0.f;
  if (h_rootflag & 1) {  // nothing has been written
    info.outcome = CLRRT_REBASE_ROOT_COLLIDES;
    HIPP(c, pre, hipEventRecord(ev1, st));
    HIPP(c, pre, hipEventSynchronize(ev1));
    HIPP(c, pre, hipEventElapsedTime(&ms, ev0, ev1));
    info.device_ms = ms;
    if (out) *out = info;
    return CLRRT_OK;
  }
  const uint64_t total = h_last[0] + h_last[1];
  const int nk = (int)(total & 0xffffffffull);
  const int64_t rows_kept = (int64_t)(total >> 32);
  const int depth = (int)h_stats[2];
  // new headers and costs, in scratch
  Scratch<clrrt_node> hdr;
  Scratch<int64_t> offs;
  Scratch<int> lvl;
  HIPP(c, pre, hdr.alloc(nk));
  HIPP(c, pre, offs.alloc(2 * (size_t)nk));
  HIPP(c, pre, lvl.alloc(nk));
  const double inf4[4] = {HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  HIPP(c, pre, hipMemcpyAsync(bbox, inf4, sizeof(inf4), hipMemcpyHostToDevice, st));
  RebaseHdr ha;
  ha.tree = c->tree; ha.n = n; ha.root = root; ha.rank = c->rank;
  ha.P0 = pose[0]; ha.P1 = pose[1]; ha.P2 = pose[2]; ha.t_shift = t_shift;
  ha.packed = packed; ha.scanned = scanned; ha.hop = hop[cur]; ha.nflag = nflag;
  ha.hdr = hdr; ha.src = offs; ha.noff = offs + nk; ha.lvl = lvl; ha.bbox = bbox; ha.err = err;
  HIPP(c, pre, launch_rebase_headers(st, ha));
  for (int level = 0; level < depth; level++)
    HIPP(c, pre, launch_rebase_cost(st, nk, level, lvl, ha.src, terms, ts, c->dp.bend, hdr));
  double h_box[4];
  HIPP(c, pre, hipMemcpyAsync(&h_err, err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipMemcpyAsync(h_box, bbox, sizeof(h_box), hipMemcpyDeviceToHost, st));
  HIPP(c, pre, hipStreamSynchronize(st));
  if (h_err != 0) return fail(c, CLRRT_ESTATE, "tree_rebase: node rows are not laid out in node order");
  // from here the tree changes: rows window by window, then headers and mirror
  pf_reset(c);
  c->rep_n = 0;
  {
    Scratch<double> win;
    const int64_t W = std::min<int64_t>(c->rebase_window_rows, rows_kept);
    HIPP(c, pre, win.alloc(10 * (size_t)W));
    RebaseMove mv;
    mv.noff = ha.noff; mv.src = ha.src; mv.nk = nk;
    mv.P0 = pose[0]; mv.P1 = pose[1]; mv.P2 = pose[2]; mv.t_shift = t_shift;
    mv.arena = c->arena; mv.win = win;
    for (int64_t w0 = 0; w0 < rows_kept; w0 += W) {
      mv.w0 = w0;
      mv.cnt = (int)std::min<int64_t>(W, rows_kept - w0);
      HIPP(c, pre, launch_rebase_move(st, mv));
    }
    HIPP(c, pre, launch_rebase_commit(st, hdr, nk, c->tree, c->nn));
    HIPP(c, pre, hipEventRecord(ev1, st));
    HIPP(c, pre, hipStreamSynchronize(st));  // (the scratch is freed on return)
  }
  HIPP(c, pre, hipEventElapsedTime(&ms, ev0, ev1));
  c->n_nodes = nk;
  c->n_rows = rows_kept;
  bbox_reset(c);  // the search frame follows the tree's new extent
  bbox_add(c, h_box[0], h_box[1], h_box[2], h_box[3]);
  info.outcome = CLRRT_REBASE_KEPT;
  info.depth = depth;
  info.nodes_kept = nk;
  info.rows_kept = rows_kept;
  info.device_ms = ms;
  if (out) *out = info;
  return CLRRT_OK;
}

int clrrt_exact_stats(clrrt_ctx* c, int64_t out[10]) {
  if (!c || !out) return CLRRT_EINVAL;
  for (int i = 0; i < 10; i++) out[i] = c->ex_stats[i];
  return CLRRT_OK;
}

int clrrt_exact_fix_hist(clrrt_ctx* c, int64_t out[16]) {
  if (!c || !out) return CLRRT_EINVAL;
  for (int i = 0; i < 16; i++) out[i] = c->ex_hist[i];
  return CLRRT_OK;
}

int clrrt_iteration_log(clrrt_ctx* c, int32_t on) {
  if (!c) return CLRRT_EINVAL;
  c->iter_log = on != 0;
  c->iters.clear();
  return CLRRT_OK;
}

int clrrt_iteration_records(clrrt_ctx* c, int64_t first, int64_t count, clrrt_iteration* out, int64_t* n_total) {
  if (!c || first < 0 || count < 0 || first + count > (int64_t)c->iters.size() || (count > 0 && !out))
    return CLRRT_EINVAL;
  if (n_total) *n_total = (int64_t)c->iters.size();
  for (int64_t i = 0; i < count; i++) out[i] = c->iters[first + i];
  return CLRRT_OK;
}

int clrrt_tree_size(clrrt_ctx* c, int64_t* n_nodes, int64_t* n_rows) {
  if (!c) return CLRRT_EINVAL;
  if (n_nodes) *n_nodes = c->n_nodes;
  if (n_rows) *n_rows = c->n_rows;
  return CLRRT_OK;
}

int clrrt_tree_download(clrrt_ctx* c, int64_t first, int64_t count, clrrt_node* out) {
  if (!c || first < 0 || count < 0 || first + count > c->n_nodes || (count > 0 && !out)) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (count == 0) return CLRRT_OK;
  HIPC(c, hipMemcpyAsync(out, c->tree + first, sizeof(clrrt_node) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_tree_rows(clrrt_ctx* c, int64_t row_offset, int64_t nrows, double* out) {
  if (!c || row_offset < 0 || nrows < 0 || row_offset + nrows > c->n_rows || (nrows > 0 && !out))
    return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (nrows == 0) return CLRRT_OK;
  int rc = flush_replays(c);
  if (rc != CLRRT_OK) return rc;
  HIPC(c, hipMemcpyAsync(out, c->arena + row_offset * 10, sizeof(double) * 10 * nrows, hipMemcpyDeviceToHost,
                         c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_extract_best_path(clrrt_ctx* c, int32_t* path, int32_t cap, int32_t* n_path, float* best_cost,
                            int64_t* n_goal) {
  if (!c || !n_path || cap < 0 || (cap > 0 && !path)) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  *n_path = 0;
  if (best_cost) *best_cost = HUGE_VALF;
  if (n_goal) *n_goal = 0;
  const int64_t n = c->n_nodes;
  if (n == 0) return CLRRT_OK;
  if (!c->bp_path) {  // allocated last: marks the pair complete
    HIPC(c, c->mem.renew(&c->goal_recs, c->cap.max_nodes));
    HIPC(c, c->mem.renew(&c->bp_path, c->cap.max_nodes + 2));
  }
  int* d_cnt = c->bp_path + c->cap.max_nodes;
  HIPC(c, launch_goal_gather(c->stream, c->tree, n, c->goal_recs, d_cnt));
  int cnt = 0;
  HIPC(c, hipMemcpyAsync(&cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (n_goal) *n_goal = cnt;
  if (cnt == 0) return CLRRT_OK;  // "No feasible path found" (rrtplanner.cpp:361-366)
  std::vector<GoalRec> g(cnt);
  HIPC(c, hipMemcpyAsync(g.data(), c->goal_recs, sizeof(GoalRec) * cnt, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  // pair_vector in tree order (rrtplanner.cpp:330-335), then the reference's sort verbatim in
  // semantics: std::sort on (id, double(costS)) pairs by .second -- equal costs keep whatever
  // order introsort leaves them in, which depends on the input order, hence the id pass first.
  std::sort(g.begin(), g.end(), [](const GoalRec& a, const GoalRec& b) { return a.id < b.id; });
  std::vector<std::pair<int, double>> pv(cnt);
  for (int i = 0; i < cnt; i++) pv[i] = std::make_pair((int)g[i].id, (double)g[i].cost);
  std::sort(pv.begin(), pv.end(),
            [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.second < b.second; });
  const int best = pv.front().first;
  if (best_cost) *best_cost = (float)pv.front().second;
  HIPC(c, launch_backtrack(c->stream, c->tree, n, best, (int)c->cap.max_nodes, c->bp_path, d_cnt + 1));
  int len = 0;
  HIPC(c, hipMemcpyAsync(&len, d_cnt + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (len <= 0) return fail(c, CLRRT_EINVAL, "extract_best_path: parent chain does not reach the root");
  const int m = std::min<int>(len, cap);
  if (m > 0) {
    std::vector<int> chain(len);  // goal -> root
    HIPC(c, hipMemcpyAsync(chain.data(), c->bp_path, sizeof(int) * len, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++) path[i] = chain[len - 1 - i];
  }
  *n_path = len;
  return CLRRT_OK;
}

// ------------------------------------------------------------------ committed path / re-init
// Grow the path buffers to hold n nodes and nrows rows (contents not preserved).
static int path_reserve(clrrt_ctx* c, int n, int64_t nrows) {
  if (n > c->path_cap) {
    const int cap = std::max(n, 2 * c->path_cap);
    c->path_cap = 0;
    HIPC(c, c->mem.renew(&c->path_nodes, cap));
    HIPC(c, c->mem.renew(&c->ri_int, 3 * (size_t)cap));
    HIPC(c, c->mem.renew(&c->ri_off, (size_t)cap + 3));
    HIPC(c, c->mem.renew(&c->ri_cost, cap));
    c->path_cap = cap;
  }
  if (nrows > c->path_rows_cap) {
    const int64_t cap = std::max<int64_t>(nrows, 2 * c->path_rows_cap);
    c->path_rows_cap = 0;
    HIPC(c, c->mem.renew(&c->path_rows, 10 * (size_t)cap));
    HIPC(c, c->mem.renew(&c->ri_terms, 2 * (size_t)cap));
    c->path_rows_cap = cap;
  }
  return CLRRT_OK;
}

int clrrt_path_commit(clrrt_ctx* c, const int32_t* ids, int32_t n, int32_t* n_remote) {
  if (!c || n < 0 || (n > 0 && !ids)) return CLRRT_EINVAL;
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= c->n_nodes) return fail(c, CLRRT_EINVAL, "path_commit: node id outside the tree");
  HIPC(c, hipSetDevice(c->device));
  int frc = flush_replays(c);  // the path's rows are copied from the arena
  if (frc != CLRRT_OK) return frc;
  if (n_remote) *n_remote = 0;
  c->path_n = 0;
  c->path_nrows = 0;
  if (n == 0) return CLRRT_OK;
  int rc = path_reserve(c, n, 1);
  if (rc != CLRRT_OK) return rc;
  // headers of the path nodes, then path-local row offsets on the host
  HIPC(c, hipMemcpyAsync(c->ri_int, ids, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
  HIPC(c, launch_gather_nodes(c->stream, c->tree, c->ri_int, n, c->path_nodes));
  std::vector<clrrt_node> h(n);
  HIPC(c, hipMemcpyAsync(h.data(), c->path_nodes, sizeof(clrrt_node) * n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  std::vector<int64_t> src(n);
  int64_t rows = 0;
  int remote = 0;
  for (int i = 0; i < n; i++) {
    if (h[i].nrows < 1) return fail(c, CLRRT_EINVAL, "path_commit: node without trajectory rows");
    src[i] = h[i].row_offset;
    h[i].row_offset = rows;
    rows += h[i].nrows;
    if (h[i].owner != c->rank) remote++;
  }
  rc = path_reserve(c, n, rows);
  if (rc != CLRRT_OK) return rc;
  HIPC(c, hipMemcpyAsync(c->path_nodes, h.data(), sizeof(clrrt_node) * n, hipMemcpyHostToDevice, c->stream));
  for (int i = 0; i < n; i++) {
    double* dst = c->path_rows + h[i].row_offset * 10;
    const size_t bytes = sizeof(double) * 10 * h[i].nrows;
    if (h[i].owner == c->rank) {
      HIPC(c, hipMemcpyAsync(dst, c->arena + src[i] * 10, bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
      HIPC(c, hipMemsetAsync(dst, 0, bytes, c->stream));
    }
  }
  HIPC(c, hipStreamSynchronize(c->stream));
  c->path_n = n;
  c->path_nrows = rows;
  if (n_remote) *n_remote = remote;
  return CLRRT_OK;
}

int clrrt_path_load(clrrt_ctx* c, const clrrt_node* nodes, int32_t n, const double* rows, int64_t n_rows) {
  if (!c || n < 0 || n_rows < 0 || (n > 0 && (!nodes || !rows))) return CLRRT_EINVAL;
  for (int i = 0; i < n; i++)
    if (nodes[i].nrows < 1 || nodes[i].row_offset < 0 || nodes[i].row_offset + nodes[i].nrows > n_rows)
      return fail(c, CLRRT_EINVAL, "path_load: node rows outside the row buffer");
  HIPC(c, hipSetDevice(c->device));
  int rc = path_reserve(c, n, n_rows);
  if (rc != CLRRT_OK) return rc;
  if (n > 0) {
    HIPC(c, hipMemcpyAsync(c->path_nodes, nodes, sizeof(clrrt_node) * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->path_rows, rows, sizeof(double) * 10 * n_rows, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
  }
  c->path_n = n;
  c->path_nrows = n > 0 ? n_rows : 0;
  return CLRRT_OK;
}

int clrrt_path_size(clrrt_ctx* c, int32_t* n, int64_t* n_rows) {
  if (!c) return CLRRT_EINVAL;
  if (n) *n = c->path_n;
  if (n_rows) *n_rows = c->path_nrows;
  return CLRRT_OK;
}

int clrrt_path_device(clrrt_ctx* c, void** dev_nodes, double** dev_rows, int32_t* n, int64_t* n_rows) {
  if (!c) return CLRRT_EINVAL;
  if (dev_nodes) *dev_nodes = c->path_n > 0 ? (void*)c->path_nodes : nullptr;
  if (dev_rows) *dev_rows = c->path_n > 0 ? c->path_rows : nullptr;
  if (n) *n = c->path_n;
  if (n_rows) *n_rows = c->path_nrows;
  return CLRRT_OK;
}

int clrrt_path_download(clrrt_ctx* c, clrrt_node* nodes, double* rows) {
  if (!c) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (c->path_n > 0 && nodes)
    HIPC(c, hipMemcpyAsync(nodes, c->path_nodes, sizeof(clrrt_node) * c->path_n, hipMemcpyDeviceToHost, c->stream));
  if (c->path_nrows > 0 && rows)
    HIPC(c, hipMemcpyAsync(rows, c->path_rows, sizeof(double) * 10 * c->path_nrows, hipMemcpyDeviceToHost,
                           c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_path_transform(clrrt_ctx* c, int32_t dir, const double pose[3]) {
  if (!c || !pose || (dir != CLRRT_WORLD_TO_CAR && dir != CLRRT_CAR_TO_WORLD)) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (c->path_n == 0) return CLRRT_OK;
  HIPC(c, launch_path_transform(c->stream, c->path_nodes, c->path_n, c->path_rows, c->path_nrows,
                                dir == CLRRT_CAR_TO_WORLD, pose));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_tree_init_from_path(clrrt_ctx* c, const double car_state[6], int32_t* outcome) {
  if (!c || !car_state) return CLRRT_EINVAL;
  pf_reset(c);
  c->rep_n = 0;  // the tree is replaced by the committed path's survivors (their rows: the path buffer)
  HIPC(c, hipSetDevice(c->device));
  int rc = path_reserve(c, std::max(1, c->path_n), std::max<int64_t>(1, c->path_nrows));
  if (rc != CLRRT_OK) return rc;
  if (c->path_n > c->cap.max_nodes || c->path_nrows > c->cap.max_rows)
    return fail(c, CLRRT_ECAPACITY, "tree_init_from_path: committed path exceeds the tree capacity");
  ReinitArgs a;
  a.p = c->dp;
  a.occ = occ_view(c);
  a.obs = c->obs;
  a.pn = c->path_nodes;
  a.n = c->path_n;
  a.prow = c->path_rows;
  for (int k = 0; k < 10; k++) a.car[k] = k < 6 ? car_state[k] : 0.0;
  a.tree = c->tree;
  a.nn = c->nn;
  a.arena = c->arena;
  a.kidx = c->ri_int;
  a.koff = c->ri_off;
  a.terms = c->ri_terms;
  a.costs = c->ri_cost;
  a.out = c->ri_off + c->path_cap;
  a.rank = c->rank;
  a.max_nodes = c->cap.max_nodes;
  a.max_rows = c->cap.max_rows;
  HIPC(c, launch_tree_reinit(c->stream, a));
  int64_t out[3];
  HIPC(c, hipMemcpyAsync(out, a.out, sizeof(out), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (out[0] < 0) return fail(c, CLRRT_ECAPACITY, "tree_init_from_path: tree capacity");
  c->n_nodes = out[1];
  c->n_rows = out[2];
  c->tree_rowless = false;
  bbox_reset(c);
  HIPC(c, launch_bbox(c->stream, c->tree, nullptr, (int)c->n_nodes, c->d_bbox));
  HIPC(c, hipMemcpyAsync(c->h_bbox, c->d_bbox, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  bbox_add(c, c->h_bbox[0], c->h_bbox[1], c->h_bbox[2], c->h_bbox[3]);
  if (outcome) *outcome = (int32_t)out[0];
  return CLRRT_OK;
}

int clrrt_path_mpc_message(clrrt_ctx* c, int32_t filtered, double* out, int32_t cap, int32_t* n_points) {
  if (!c || !n_points || cap < 0 || (cap > 0 && !out)) return CLRRT_EINVAL;
  *n_points = 0;
  if (c->path_n == 0) return CLRRT_OK;
  std::vector<clrrt_node> h(c->path_n);
  std::vector<double> rows(10 * c->path_nrows);
  int rc = clrrt_path_download(c, h.data(), rows.data());
  if (rc != CLRRT_OK) return rc;
  // generateMPCmessage: rows 1 .. nrows-1 of every segment
  std::vector<std::array<double, 8>> msg;
  for (const clrrt_node& nd : h)
    for (int i = 1; i < nd.nrows; i++) {
      const double* r = &rows[(nd.row_offset + i) * 10];
      msg.push_back({r[0], r[1], r[2], r[3], r[4], r[5], r[8], r[9]});
    }
  if (filtered && !msg.empty()) {  // filterMPCmessage: keep index i when the distance since the last kept is 0
    std::vector<std::array<double, 8>> f;
    const double interval = 5;
    double d = 0;
    for (size_t i = 1; i != msg.size(); i++) {
      if (d == 0) {
        std::array<double, 8> p = msg[i];
        p[3] = NAN;
        f.push_back(p);
      }
      const double dx = msg[i][0] - msg[i - 1][0], dy = msg[i][1] - msg[i - 1][1];
      d += sqrt(dx * dx + dy * dy);
      if (d >= interval) d = 0;
    }
    msg.swap(f);
  }
  *n_points = (int32_t)msg.size();
  for (int i = 0; i < (int)msg.size() && i < cap; i++)
    for (int k = 0; k < 8; k++) out[8 * i + k] = msg[i][k];
  return CLRRT_OK;
}

int clrrt_get_counters(clrrt_ctx* c, clrrt_counters* out) {
  if (!c || !out) return CLRRT_EINVAL;
  *out = c->counters;
  return CLRRT_OK;
}

int clrrt_reset_counters(clrrt_ctx* c) {
  if (!c) return CLRRT_EINVAL;
  memset(&c->counters, 0, sizeof(c->counters));
  c->nn_bf_keys = c->nn_samples = c->nn_super_bounds = 0;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemsetAsync(c->work_ctr, 0, 64 * sizeof(unsigned long long), c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_debug_counters(clrrt_ctx* c, int64_t out[64]) {
  if (!c || !out) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  unsigned long long h[64];
  HIPC(c, hipMemcpy(h, c->work_ctr, sizeof(h), hipMemcpyDeviceToHost));
  for (int i = 0; i < 64; i++) out[i] = (int64_t)h[i];
  return CLRRT_OK;
}

// Guard bands around every block of this library's memory owner (clrrt::MemGuard, clrrt_devmem.hpp): a test facility.
int clrrt_debug_mem_guard(int64_t bytes) {
  if (bytes < 0 || !clrrt::MemGuard<HipMem>::set((size_t)bytes)) return CLRRT_EINVAL;
  return CLRRT_OK;
}

int clrrt_debug_mem_check(clrrt_mem_report* out) {
  if (!out) return CLRRT_EINVAL;
  clrrt::MemReport r;
  clrrt::MemGuard<HipMem>::check(&r);  // (each band's copy-out waits for the device first)
  *out = clrrt_mem_report{r.blocks_checked, r.guard_bytes_checked, r.violations, r.first_serial,
                          r.first_bytes,    r.first_offset,        r.first_side, 0};
  return CLRRT_OK;
}

int clrrt_work_counters(clrrt_ctx* c, int64_t out[3]) {
  if (!c || !out) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  unsigned long long h[4];
  HIPC(c, hipMemcpyAsync(h, c->work_ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 3; i++) out[i] = (int64_t)h[i];
  return CLRRT_OK;
}

int clrrt_search_work(clrrt_ctx* c, int64_t out[4]) {
  if (!c || !out) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (c->side) HIPC(c, hipStreamSynchronize(c->side));
  unsigned long long h[19];
  HIPC(c, hipMemcpy(h, c->work_ctr + 8, sizeof(h), hipMemcpyDeviceToHost));
  out[0] = c->nn_bf_keys;
  out[1] = c->nn_samples;
  out[2] = (int64_t)h[11];
  out[3] = (int64_t)h[13];
  return CLRRT_OK;
}

int clrrt_search_work_ex(clrrt_ctx* c, int64_t out[8]) {
  if (!c || !out) return CLRRT_EINVAL;
  int64_t w[4];
  const int rc = clrrt_search_work(c, w);
  if (rc != CLRRT_OK) return rc;
  unsigned long long h[19];
  HIPC(c, hipMemcpy(h, c->work_ctr + 8, sizeof(h), hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; i++) out[i] = w[i];
  out[4] = c->nn_super_bounds;
  out[5] = (int64_t)h[10];  // super-tile visits (32 tile bounds each)
  out[6] = (int64_t)h[12];  // records past the prefilter (queued for stage 1 / 2)
  out[7] = 0;
  return CLRRT_OK;
}

int clrrt_nn_stats(clrrt_ctx* c, int64_t out[19]) {
  if (!c || !out) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  unsigned long long h[19];
  HIPC(c, hipMemcpy(h, c->work_ctr + 8, sizeof(h), hipMemcpyDeviceToHost));
  for (int i = 0; i < 19; i++) out[i] = (int64_t)h[i];
  out[4] &= 0xffffffff;
  return CLRRT_OK;
}

int clrrt_set_option(clrrt_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return CLRRT_EINVAL;
  const std::string k(key);
  if (k == "roll_persistent") c->roll_persistent = value != 0;
  else if (k == "nn_walk_min" && value >= 0) c->nnw_min_nodes = value;
  else if (k == "nn_walk_stateless") c->nnw_stateless = value != 0;
  else if (k == "nn_walk_budget_tiles" && value >= 0 && value < INT_MAX) {
    c->nnw_bud_tiles = (int)value;
    c->nnw_bud_tiles_set = true;
  }
  else if (k == "nn_walk_budget_keys" && value >= 0 && value < INT_MAX) c->nnw_bud_ex = (int)value;
  else if (k == "nn_walk_half_max" && value >= 0 && value < INT_MAX) c->nnw_half_max = (int)value;
  else if (k == "nn_walk_hscale" && value >= 1 && value <= 10000) {  // index order: scheduling only
    c->nnw_hscale = (int)value;
    c->nnw_built.n = -1;
    c->nnw.sorted_n = c->nnw_alt.sorted_n = c->nnw3.sorted_n = -1;
  }
  else if (k == "nn_root_seed" || (k == "nn_root_k" && value >= 1 && value <= 64) ||
           (k == "nn_root_scan" && value >= 1 && value <= 32768)) {  // same lists; a kept index has the old marks
    if (k == "nn_root_seed") c->nnw_root_seed = value != 0;
    else if (k == "nn_root_k") c->nnw_root_k = (int)value;
    else c->nnw_root_scan = (int)value;
    c->nnw_built.n = -1;
  }
  else if (k == "nn_walk_index" && value >= 0 && value <= 5) {
    c->nnw_index = (int)value;
    c->nnw_built.n = -1;  // the kept index and sort results have the old order
    c->nnw.sorted_n = c->nnw_alt.sorted_n = c->nnw3.sorted_n = -1;
  }
  else if (k == "nn_walk_waves" && value >= -1 && value <= 1 << 20) c->nnw_waves = (int)value;
  else if (k == "nn_walk_chunks" && value >= 1 && value <= kWalkMaxChunks) c->nnw_chunks = (int)value;
  else if (k == "nn_walk_max_over" && value >= 1 && value <= kWalkMaxOver) {
    c->nnw_max_over = (int)value;
    c->nnw_max_over_set = true;
  }
  else if (k == "nn_walk_double") c->nnw_double = value != 0;
  else if (k == "nn_lag" && (value == 0 || value == 1 || value == 2)) c->nn_lag = (int)value;
  else if (k == "nn_delta_walk") c->nn_delta_walk = value != 0 ? 1 : 0;  // same lists either way
  else if (k == "nn_delta_verify") c->nn_delta_verify = value != 0 ? 1 : 0;  // diagnostics: counters 38 / 39
  else if (k == "nn_debug" && value >= 0) c->nn_debug = (int)value;  // diagnostics: changes results
  else if (k == "fail_at_round" && value >= 0 && value < INT_MAX) c->fail_at_round = (int)value;  // fault injection
  else if (k == "fail_after_exchange" && value >= 0 && value < INT_MAX) c->fail_after_exchange = (int)value;
  else if (k == "fail_in_round" && value >= 0 && value < INT_MAX) c->fail_in_round = (int)value;
  else if (k == "shard_hook_world1") c->sh.hook_world1 = value != 0;  // read by the next clrrt_set_shards
  else if (k == "roll_blocks" && value >= 0 && value < (1 << 20)) c->roll_blocks = (int)value;
  else if (k == "nn_pipeline") c->nn_pipeline = value != 0;
  else if (k == "roll_priority") c->roll_priority = value != 0;
  else if (k == "roll_order_verify") c->roll_order_verify = value != 0;  // diagnostics: counters 6 / 7
  else if (k == "roll_coop") c->roll_coop = value != 0;
  else if (k == "roll_spread") c->roll_spread = value != 0;
  else if (k == "roll_lanes") c->roll_lanes = (int)std::max<int64_t>(0, std::min<int64_t>(64, value));
  else if (k == "nn_exact_fused") c->nn_exact_fused = value != 0;
  else if (k == "rows_deferred") {
    int rc = flush_replays(c);
    if (rc != CLRRT_OK) return rc;
    c->rows_deferred = value != 0;
  }
  else if (k == "exact_min_width" && value >= 1 && value <= 1 << 20) c->exact_min_width = (int)value;
  else if (k == "exact_fixup") c->exact_fixup = value != 0;
  else if (k == "exact_fixup_cap" && value >= 0 && value < INT_MAX) c->exact_fix_cap = (int)value;
  else if (k == "defer_steps" && value >= 0 && value <= 1 << 20) {
    // BATCH rounds with deferred samples (changes the BATCH tree: samples whose rollouts run past T steps
    // per launch commit in a later round, by a deterministic rule the oracle restates); 0 = off
    if (value > 0 && value < 8) return fail(c, CLRRT_EINVAL, "defer_steps must be 0 or >= 8");
    c->def.T = (int)value;
  }
  else if (k == "stream_prio") c->stream_prio = value != 0;
  // clrrt_tree_rebase moves rows through a scratch window of this many rows (at most 64 MiB; results do not depend on it)
  else if (k == "rebase_window_rows" && value >= 1 && value <= 838860) c->rebase_window_rows = value;
  else return fail(c, CLRRT_EINVAL, "unknown option or value: " + k);
  return CLRRT_OK;
}

int clrrt_enable_timing(clrrt_ctx* c, int32_t on) {
  if (!c) return CLRRT_EINVAL;
  drain_timers(c);
  c->timing = on != 0;
  for (int i = 0; i < clrrt_ctx::kKtClasses; i++) { c->kt_ms[i] = 0; c->kt_n[i] = 0; }
  return CLRRT_OK;
}

int clrrt_kernel_time(clrrt_ctx* c, int32_t which, double* ms, int64_t* launches) {
  if (!c || which < 0 || which >= clrrt_ctx::kKtClasses) return CLRRT_EINVAL;
  drain_timers(c);
  if (ms) *ms = c->kt_ms[which];
  if (launches) *launches = c->kt_n[which];
  return CLRRT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ rounds
static RollArgs roll_args(clrrt_ctx* c, int njobs) {
  RollArgs a;
  memset(&a, 0, sizeof(a));
  ListSet& cur = *c->ls[0];
  a.p = c->dp;
  a.tree = c->tree;
  a.samples = cur.d_samples;
  a.cand = cur.cand;
  a.jobs = c->jobs;
  a.obs = c->obs;
  a.arena = c->arena;
  a.ctr = c->work_ctr;
  a.grid = c->grid;
  a.occ = occ_view(c);
  a.njobs = njobs;
  return a;
}

static int ensure_sort_scratch(clrrt_ctx* c, int64_t entries) {
  if (entries <= c->sort_cap) return CLRRT_OK;
  HIPC(c, hipStreamSynchronize(c->stream));
  c->sort_cap = 0;
  int64_t want = std::max<int64_t>(entries, 1 << 20);
  HIPC(c, c->mem.renew(&c->sort_scratch, want));
  c->sort_cap = want;
  return CLRRT_OK;
}

// One walk-search buffer set, sized for the context's capacity.
static int alloc_walk(clrrt_ctx* c, WalkBufs& w) {
  if (w.P) return CLRRT_OK;
  const int64_t M = std::max<int64_t>(c->cap.max_nodes, c->cap.max_batch);
  const int64_t Mp = c->cap.max_nodes + 1024;
  HIPC(c, c->mem.renew(&w.sorder, c->cap.max_batch));
  HIPC(c, c->mem.renew(&w.keys, 2 * M));
  HIPC(c, c->mem.renew(&w.keys2, 2 * M));
  HIPC(c, c->mem.renew(&w.vals, std::max<int64_t>(M, Mp)));  // also the run markers of the padded records
  HIPC(c, c->mem.renew(&w.vals2, M));
  w.tmp_bytes = walk_sort_bytes((int)M);
  HIPC(c, c->mem.renew_bytes(&w.tmp, std::max<size_t>(w.tmp_bytes, 256)));
  HIPC(c, c->mem.renew(&w.Q, Mp));
  HIPC(c, c->mem.renew(&w.CE, Mp));
  HIPC(c, c->mem.renew(&w.ID, Mp));
  HIPC(c, c->mem.renew(&w.HEAD, Mp));
  HIPC(c, c->mem.renew(&w.trun, walk_tile_count(c->cap.max_nodes) + 1));
  // one record per tile / super-tile of the padded index (launch_nn_walk_build)
  HIPC(c, c->mem.renew(&w.tiles, walk_tile_count(c->cap.max_nodes) + 1));
  HIPC(c, c->mem.renew(&w.supers, walk_super_count(c->cap.max_nodes) + 1));
  HIPC(c, c->mem.renew(&w.ovf_n, 1));
  HIPC(c, c->mem.renew(&w.ovf, kWalkMaxOver));
  HIPC(c, c->mem.renew(&w.wctr, 8 + 2 + 64));  // + the root roster (count, X, 64 ids)
  w.roster = w.wctr + 8;
  HIPC(c, c->mem.renew(&w.pk, (int64_t)kWalkMaxOver * kWalkMaxChunks * 11));
  HIPC(c, c->mem.renew(&w.pi, (int64_t)kWalkMaxOver * kWalkMaxChunks * 11));
  HIPC(c, c->mem.renew(&w.skeys, Mp));
  HIPC(c, c->mem.renew(&w.sids, Mp));
  w.sorted_n = -1;
  w.cap_nodes = c->cap.max_nodes;
  w.cap_batch = (int)c->cap.max_batch;
  HIPC(c, c->mem.renew(&w.P, Mp));  // last: marks the set complete
  return CLRRT_OK;
}

// Walk-search configuration of a set (+ its buffers on first use).
static int ensure_walk_set(clrrt_ctx* c, WalkBufs& w) {
  w.bud_tiles = c->nnw_bud_tiles_set || c->nnw_bud_tiles == 0
                    ? c->nnw_bud_tiles
                    : (int)std::max<int64_t>(c->nnw_bud_tiles, c->n_nodes >> 11);
  // the exact-key budget grows with the tree (denser trees: more near-tied keys per sample; the cfg3
  // sweeps: 4096 best at <= 1.6 M nodes, 8192 at 4.7 M, where 4096 overflows more samples than there
  // are records)
  w.bud_ex = c->nnw_bud_ex > 0 ? (int)std::max<int64_t>(c->nnw_bud_ex, c->n_nodes >> 9) : 0;
  w.max_over = c->nnw_max_over_set || c->n_nodes < (6 << 20) ? c->nnw_max_over : kWalkMaxOver;
  w.nch = c->nnw_chunks;
  w.half_max = c->nnw_half_max;
  w.index_kind = c->nnw_index;
  w.hscale_pct = c->nnw_hscale;
  w.root_seed = c->nnw_root_seed;
  w.root_k = c->nnw_root_k;
  w.root_scan = c->nnw_root_scan;
  w.waves = c->nnw_waves < 0 ? 9 * c->n_cu : c->nnw_waves;
  // the default grid serves batches of >= 4x its waves (cfg2's 4096-sample rounds run 4% faster with one
  // wave per sample: 1.237 vs 1.188 M nodes/s)
  w.waves_min_batch = c->nnw_waves < 0 ? 4 * w.waves : 0;
  return alloc_walk(c, w);
}
static int ensure_walk(clrrt_ctx* c) { return ensure_walk_set(c, c->nnw); }

static NnSetup nn_setup(clrrt_ctx* c) {
  NnSetup su;
  double& x0 = su.x0; double& y0 = su.y0; double& x1 = su.x1; double& y1 = su.y1;
  sample_region(c->params, x0, y0, x1, y1);
  if (c->bbox[0] <= c->bbox[2]) {  // grid covers the samples and every finite node: no overflow
    x0 = std::min(x0, c->bbox[0] - 1.0); y0 = std::min(y0, c->bbox[1] - 1.0);
    x1 = std::max(x1, c->bbox[2] + 1.0); y1 = std::max(y1, c->bbox[3] + 1.0);
  }
  // float frame of the brute-force prune: |coordinate - origin| <= E for every sample and finite node
  // (samples of this round lie in the sample region, nodes in the tree's box); each float rounding
  // of a coordinate difference errs by <= 2^-24 E, a squared distance difference by a few of them
  NnFrame fr;
  fr.debug = c->nn_debug;
  fr.ox = 0.5 * (x0 + x1);
  fr.oy = 0.5 * (y0 + y1);
  {
    const double E = std::max(x1 - x0, y1 - y0) + 1.0;
    const double d = 16.0 * std::ldexp(E, -24) + 1e-5;
    fr.delta = std::isfinite(d) ? (float)d : HUGE_VALF;
  }
  su.fr = fr;
  const double W = x1 - x0, H = y1 - y0;
  su.region_ok = std::isfinite(W * H) && W * H > 0;
  return su;
}

// The walk search serves the tree as it is now (run_nn's choice).
static bool walk_serves(clrrt_ctx* c, const NnSetup& su) {
  return c->n_nodes >= c->nnw_min_nodes && su.region_ok;
}

// Any tree change other than clrrt_round_commit invalidates a prefetched search.
// (pf_discard: the prefetch alone -- the calls that overwrite the list buffers without changing the tree)
static void pf_discard(clrrt_ctx* c) {
  if (c->pf_state != 0 && c->side) hipStreamSynchronize(c->side);
  c->pf_state = 0;
  c->pf_next.clear();
}
static void pf_reset(clrrt_ctx* c) {
  pf_discard(c);
  c->nnr_built.n = -1;
  c->nnw_built.n = -1;
  c->nnw.sorted_n = -1;  // the kept sort results describe the old tree
  c->nnw_alt.sorted_n = -1;
  c->nnw3.sorted_n = -1;
}

// The pipelined rounds' indexes cover the whole tree as it is now, under the current index options.
static bool tree_index_matches(const clrrt_ctx* c, const BuiltFor& b, const NnSetup& su) {
  return b.matches(c->n_nodes, 0, c->n_nodes, su, c->nnw_index, c->nnw_hscale);
}
static void tree_index_set(const clrrt_ctx* c, BuiltFor& b, const NnSetup& su) {
  b.set(c->n_nodes, 0, c->n_nodes, su, c->nnw_index, c->nnw_hscale);
}
// The index is built on the main stream before the rollouts (its radix sort's look-back passes starve
// beside the rollout kernel on large trees: 3+ ms instead of 0.2), the search runs on the side stream.
static int pre_roll_build(clrrt_ctx* c, const NnSetup& su) {
  KTimer kt(c, 0, c->stream);
  const int rw = ensure_walk(c);
  if (rw != CLRRT_OK) return rw;
  if (tree_index_matches(c, c->nnw_built, su)) return CLRRT_OK;  // built ahead (next_round_build)
  HIPC(c, launch_nn_walk_build(c->stream, c->nn, (int)c->n_nodes, su.fr, su.x0, su.y0, su.x1, su.y1, c->nnw,
                               c->nnw_alt.P ? &c->nnw_alt : nullptr));
  tree_index_set(c, c->nnw_built, su);
  return CLRRT_OK;
}

// Pipelined rounds, right after a commit: the next round's index over the committed tree goes into
// the other buffer set on the main stream while the side stream's search still reads this one (it
// waits for nothing but the commit; the wait for the side search comes after it).
static int next_round_build(clrrt_ctx* c) {
  const NnSetup su = nn_setup(c);
  if (!walk_serves(c, su)) return CLRRT_OK;
  std::swap(c->nnw, c->nnw_alt);
  c->nnw_built.n = -1;
  return pre_roll_build(c, su);
}

// Launches the walk search of the n2 samples in ls[1]'s host copy over the current tree on the side
// stream into that set; eval_samples records ev_tree before its rollouts.
static int launch_side_walk(clrrt_ctx* c, int n2, const NnSetup& su) {
  ListSet& nxt = *c->ls[1];
  c->nn_bf_keys += (int64_t)n2 * c->n_nodes;
  c->nn_samples += n2;
  HIPC(c, hipStreamWaitEvent(c->side, c->ev_tree, 0));
  HIPC(c, hipMemcpyAsync(nxt.d_samples, nxt.h_samples, sizeof(clrrt_sample) * n2, hipMemcpyHostToDevice, c->side));
  c->nn_super_bounds += (int64_t)n2 * walk_super_count(c->n_nodes);
  {
    KTimer kt(c, 0, c->side), kt3(c, 3, c->side);
    HIPC(c, launch_nn_walk_search(c->side, nxt.d_samples, n2, c->nn, (int)c->n_nodes, c->dp, su.fr, su.x0, su.y0,
                                  su.x1, su.y1, c->nnw, nxt.cand, nxt.ckey, nxt.ncand, nxt.ctie, c->work_ctr + 18,
                                  c->nnw_stateless));
  }
  HIPC(c, hipEventRecord(c->ev_walk, c->side));
  return CLRRT_OK;
}

// After the appended nodes [first_new, first_new + nn) are in the tree (queued on the main stream):
// their search for the next round's samples, merged into the side walk's lists, runs on the side
// stream behind the walk, so the main stream can build the next round's index meanwhile.
static int side_delta_launch(clrrt_ctx* c, int n2, int64_t first_new, int nn) {
  if (nn <= 0) return CLRRT_OK;
  ListSet& nxt = *c->ls[1];
  HIPC(c, hipEventRecord(c->ev_commit, c->stream));
  HIPC(c, hipStreamWaitEvent(c->side, c->ev_commit, 0));
  {
    KTimer kt(c, 0, c->side);
    c->nn_bf_keys += (int64_t)n2 * nn;
    const NnSetup su2 = nn_setup(c);  // the box includes the appended nodes
    const int max_chunks = (int)std::max<int64_t>(1, c->partial_cap / ((int64_t)n2 * NN_K));
    HIPC(c, launch_nn_delta(c->side, nxt.d_samples, n2, c->nn, (int)first_new, nn, c->dp, su2.fr, c->pk, c->pi,
                            max_chunks, nxt.cand, nxt.ckey, nxt.ncand, nxt.ctie, c->nn_seed));
  }
  HIPC(c, hipEventRecord(c->ev_walk, c->side));
  return CLRRT_OK;
}

// The main stream waits for the side stream's lists and their set becomes the current one.
static int side_lists_join(clrrt_ctx* c) {
  {
    KTimer kt(c, 4);  // the lists' wait (time the main stream stalls on the side stream)
    HIPC(c, hipStreamWaitEvent(c->stream, c->ev_walk, 0));
  }
  std::swap(c->ls[0], c->ls[1]);
  return CLRRT_OK;
}

static int merge_side_lists(clrrt_ctx* c, int n2, int64_t first_new, int nn) {
  const int rc = side_delta_launch(c, n2, first_new, nn);
  return rc != CLRRT_OK ? rc : side_lists_join(c);
}

// Stage 1: candidate lists of samples cur.d_samples[0..n) (spatial index for large trees).
static int run_nn(clrrt_ctx* c, int n, KeyId* scratch) {
  hipStream_t st = c->stream;
  ListSet& cur = *c->ls[0];
  KTimer kt(c, 0);
  c->nn_bf_keys += (int64_t)n * c->n_nodes;
  c->nn_samples += n;
  int max_chunks = (int)std::max<int64_t>(1, c->partial_cap / ((int64_t)n * NN_K));
  if (scratch && c->nn_exact_fused && c->n_nodes <= nn_exact_small_max()) {  // EXACT rounds on small trees
    HIPC(c, launch_nn_exact_small(st, cur.d_samples, n, c->nn, (int)c->n_nodes, c->dp, cur.cand, cur.ckey, cur.ncand,
                                  cur.ctie));
    return CLRRT_OK;
  }
  const NnSetup su = nn_setup(c);
  if (walk_serves(c, su)) {
    int rc = ensure_walk(c);
    if (rc != CLRRT_OK) return rc;
    c->nnw_built.n = -1;
    HIPC(c, launch_nn_walk(st, cur.d_samples, n, c->nn, (int)c->n_nodes, c->dp, su.fr, su.x0, su.y0, su.x1, su.y1,
                           c->nnw, cur.cand, cur.ckey, cur.ncand, cur.ctie, c->work_ctr + 18, c->nnw_stateless));
    if (scratch) HIPC(c, launch_nn_exact_any(st, cur.d_samples, n, c->nn, (int)c->n_nodes, c->dp, cur.ctie, scratch,
                                              cur.cand, cur.ckey, cur.ncand));
    return CLRRT_OK;
  }
  HIPC(c, launch_nn(st, cur.d_samples, n, c->nn, (int)c->n_nodes, c->dp, c->pk, c->pi, cur.cand, cur.ckey,
                    cur.ncand, cur.ctie, max_chunks, scratch, c->nn_seed, c->work_ctr + 8, su.fr));
  return CLRRT_OK;
}

// EXACT mode, stage 5 with fix-ups (k_conflict_fix): the committed prefix of the round's n samples runs up to the
// first sample whose result the reference would not reproduce.  A sample k_conflict_fix resolves takes the fix-up
// rollouts of the new nodes that enter its list before its result; a sample it cannot resolve (ties, thresholds,
// window changes) gets its list recomputed over the tree the reference's sort sees for it -- the N tree nodes and
// the round's new nodes before it, std::sort's tie order included (launch_nn_exact_x) -- and the candidates that
// list tries before its result which the speculative evaluation did not try (new nodes, or old ones it ordered
// after its result) become fix-ups too.  The fix-ups run in one launch (one job per wave); a sample stands when all
// of its fix-ups fail and its result is still the first success of its list; its counters become those of the
// list's tried candidates.  *L: the prefix.
static int exact_fixups(clrrt_ctx* c, int n, int* L) {
  hipStream_t st = c->stream;
  ListSet& cur = *c->ls[0];
  const int64_t B = c->cap.max_batch;
  const int K = CAND_K;
  if (!c->fix_n) {
    HIPC(c, c->mem.renew(&c->fix_n, B));
    HIPC(c, c->mem.renew(&c->fix_ids, B * FIX_MAX));
    HIPC(c, c->mem.renew(&c->fix_adj, B * FIX_ADJ));
    HIPC(c, c->mem.renew(&c->fix_jobs, B * K));
    HIPC(c, c->mem.renew(&c->fix_res, B * K));
    HIPC(c, c->mem.renew(&c->fix_xrec, 2 * B));
    HIPC(c, c->mem.renew(&c->fix_xi, 2 * B));
    HIPC(c, c->mem.renew(&c->fix_xcand, B * K));
    HIPC(c, c->mem.renew(&c->fix_xkey, B * K));
    HIPC(c, c->mem.renew(&c->fix_xn, 2 * B));
  }
  {
    KTimer kt(c, 2);
    HIPC(c, launch_conflict_fix(st, c->dp, n, cur.d_samples, c->regnodes, c->gbnodes, c->so, cur.ctie, cur.ncand, cur.ckey,
                                c->res_spec, c->fix_n, c->fix_ids, c->fix_adj));
  }
  c->h_fix.resize((size_t)n * (1 + FIX_MAX + FIX_ADJ));
  c->h_fix_smp.resize(n);
  c->h_fix_so.resize(n);
  c->h_fix_cand.resize((size_t)n * K);
  c->h_fix_spec.resize((size_t)n * K);
  HIPC(c, hipMemcpyAsync(c->h_fix.data(), c->fix_n, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIPC(c, hipMemcpyAsync(c->h_fix.data() + n, c->fix_ids, sizeof(int) * n * FIX_MAX, hipMemcpyDeviceToHost, st));
  HIPC(c, hipMemcpyAsync(c->h_fix.data() + n * (1 + FIX_MAX), c->fix_adj, sizeof(int) * n * FIX_ADJ, hipMemcpyDeviceToHost,
                         st));
  HIPC(c, hipMemcpyAsync(c->h_fix_smp.data(), cur.d_samples, sizeof(clrrt_sample) * n, hipMemcpyDeviceToHost, st));
  HIPC(c, hipMemcpyAsync(c->h_fix_so.data(), c->so, sizeof(SampleOut) * n, hipMemcpyDeviceToHost, st));
  HIPC(c, hipMemcpyAsync(c->h_fix_cand.data(), cur.cand, sizeof(int) * n * K, hipMemcpyDeviceToHost, st));
  HIPC(c, hipMemcpyAsync(c->h_fix_spec.data(), c->res_spec, sizeof(RollRes) * n * K, hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  const int* fn = c->h_fix.data();
  const int* fid = c->h_fix.data() + n;
  const int* fadj = c->h_fix.data() + n * (1 + FIX_MAX);
  const int64_t N = c->n_nodes;
  // the round's new nodes in commit order: count before each sample, and (sample, 0 regular | 1 goal-biased) by position
  std::vector<int> xpre(n + 1, 0);
  std::vector<int> xpos;
  for (int k = 0; k < n; k++) {
    const SampleOut& o = c->h_fix_so[k];
    xpre[k + 1] = xpre[k];
    if (o.k >= 0) {
      xpos.push_back(2 * k);
      xpre[k + 1]++;
      if (o.gb_ok) { xpos.push_back(2 * k + 1); xpre[k + 1]++; }
    }
  }
  // the samples that need their list recomputed (and whether that fits the LDS kernel)
  const bool x_fits = N + xpre[n] <= nn_exact_small_max() && c->dp.sort_limit <= K;
  int stop = n;
  int not_found = -1;          // (diagnostics) the sample whose recomputed list no longer holds its result
  std::vector<int> xl;
  for (int j = 0; j < n; j++) {
    if (fn[j] >= 0) continue;
    if (!x_fits) { stop = j; if (-fn[j] >= 1 && -fn[j] <= 4) c->ex_stats[4 + -fn[j]]++; break; }
    xl.push_back(j);
  }
  const int nl = (int)xl.size();
  std::vector<int> xc, xn;
  if (nl > 0) {
    std::vector<int> xs(2 * nl);
    for (int i = 0; i < nl; i++) { xs[i] = xl[i]; xs[nl + i] = xpre[xl[i]]; }
    HIPC(c, hipMemcpyAsync(c->fix_xi, xs.data(), sizeof(int) * 2 * nl, hipMemcpyHostToDevice, st));
    {
      KTimer kt(c, 0);
      HIPC(c, launch_nn_exact_x(st, cur.d_samples, c->nn, (int)N, c->dp, c->regnodes, c->gbnodes, c->so, n, c->fix_xrec,
                                c->fix_xi, c->fix_xi + nl, nl, xpre[n], c->fix_xcand, c->fix_xkey, c->fix_xn,
                                c->fix_xn + nl));
    }
    xc.resize((size_t)nl * K);
    xn.resize(nl);
    HIPC(c, hipMemcpyAsync(xc.data(), c->fix_xcand, sizeof(int) * nl * K, hipMemcpyDeviceToHost, st));
    HIPC(c, hipMemcpyAsync(xn.data(), c->fix_xn, sizeof(int) * nl, hipMemcpyDeviceToHost, st));
    HIPC(c, hipStreamSynchronize(st));
  }
  auto is_fail = [](int oc) { return oc >= 0 && oc != CLRRT_ROLL_END && oc != CLRRT_ROLL_GOAL; };
  auto add_res = [](SampleOut& d, const RollRes& r, int sign) {
    d.rollouts += sign;
    d.steps += sign * (r.nrows - 1);
    d.f_col += sign * (r.outcome == CLRRT_ROLL_COLLISION);
    d.f_acc += sign * (r.outcome == CLRRT_ROLL_ACCLIMIT);
    d.f_it += sign * (r.outcome == CLRRT_ROLL_ITERLIMIT);
  };
  // per sample: the fix-up jobs and the counters' change apart from them
  c->h_fix_jobs.clear();
  c->h_fix_owner.clear();
  std::vector<SampleOut> delta(n);
  auto job = [&](int j, int from, int parent) {
    Job jb;
    jb.parent = parent;
    jb.from_reg = from;
    jb.gb = 0;
    jb.pad = 0;
    jb.sx = c->h_fix_smp[j].x;
    jb.sy = c->h_fix_smp[j].y;
    jb.row_off = -1;
    c->h_fix_jobs.push_back(jb);
    c->h_fix_owner.push_back(j);
  };
  for (int j = 0, xi = 0; j < stop; j++) {
    SampleOut& d = delta[j];
    d = SampleOut{};
    if (fn[j] >= 0) {
      for (int i = 0; i < fn[j]; i++) {
        const int id = fid[j * FIX_MAX + i];
        job(j, 1 + (id & 1), id >> 1);
      }
      const int* ad = fadj + FIX_ADJ * j;  // old candidates pushed out of the window (samples without a result)
      d.rollouts += ad[0]; d.steps += ad[1]; d.f_col += ad[2]; d.f_acc += ad[3]; d.f_it += ad[4];
      continue;
    }
    // the recomputed list
    const SampleOut& o = c->h_fix_so[j];
    const int* lst = xc.data() + (size_t)xi * K;
    const int ln = xn[xi];
    xi++;
    const int* spec = c->h_fix_cand.data() + (size_t)j * K;
    const RollRes* sres = c->h_fix_spec.data() + (size_t)j * K;
    const int acc = o.k >= 0 ? spec[o.k] : -1;
    // the speculative counters of the candidates tried before the result (all of them without one) come out ...
    for (int q = 0; q < K; q++) {
      if (spec[q] < 0 || (o.k >= 0 && q >= o.k)) break;
      add_res(d, sres[q], -1);
    }
    // ... and those of the recomputed list's candidates before the result go in (known failures, or fix-ups)
    bool found = false;
    for (int t = 0; t < ln; t++) {
      const int e = lst[t];
      if (e == acc) { found = true; break; }
      int q = -1;
      if (e < N)
        for (int r = 0; r < K && spec[r] >= 0; r++)
          if (spec[r] == e) { q = r; break; }
      if (q >= 0 && (o.k < 0 || q < o.k) && is_fail(sres[q].outcome)) {
        add_res(d, sres[q], +1);
      } else if (e < N) {
        job(j, 0, e);
      } else {
        const int pw = xpos[e - N];
        job(j, 1 + (pw & 1), pw >> 1);
      }
    }
    if (o.k >= 0 && !found) {  // the result is not its list's first success any more
      stop = j;
      not_found = j;
      c->ex_stats[8]++;
      while (!c->h_fix_owner.empty() && c->h_fix_owner.back() == j) {
        c->h_fix_owner.pop_back();
        c->h_fix_jobs.pop_back();
      }
      break;
    }
  }
  const int nj = (int)c->h_fix_jobs.size();
  c->h_fix_res.resize(nj);
  if (nj > 0) {
    HIPC(c, hipMemcpyAsync(c->fix_jobs, c->h_fix_jobs.data(), sizeof(Job) * nj, hipMemcpyHostToDevice, st));
    RollArgs a = roll_args(c, nj);
    a.jobs = c->fix_jobs;
    a.res = c->fix_res;
    a.res_gb = c->fix_res;  // (SRC_LIST runs no goal-biased pass)
    a.xreg = c->regnodes;
    a.xgb = c->gbnodes;
    a.job_stride = 64;  // one job per wave: the fix-ups run at the lone lane's step latency
    if (c->exact_fix_cap > 0 && c->exact_fix_cap < a.p.n_steps_max) a.p.n_steps_max = c->exact_fix_cap;
    {
      KTimer kt(c, 1);
      HIPC(c, launch_rollout(st, SRC_LIST, a));
    }
    HIPC(c, hipMemcpyAsync(c->h_fix_res.data(), c->fix_res, sizeof(RollRes) * nj, hipMemcpyDeviceToHost, st));
    HIPC(c, hipStreamSynchronize(st));
  }
  // in sample order: a fix-up that succeeds changes the sample's result (it ends the prefix)
  int Lr = stop, resolved = 0;
  bool patched = false;
  const int cap = c->exact_fix_cap > 0 && c->exact_fix_cap < c->dp.n_steps_max ? c->exact_fix_cap : 0;
  for (int j = 0, q = 0; j < stop; j++) {
    SampleOut add = delta[j];
    bool ok = true, any = fn[j] != 0;
    for (; q < nj && c->h_fix_owner[q] == j; q++) {
      const RollRes& r = c->h_fix_res[q];
      // (a capped rollout stopped at the cap: undecided -- the true iteration limit lies beyond it)
      if (!is_fail(r.outcome) || (cap && r.outcome == CLRRT_ROLL_ITERLIMIT)) ok = false;
      add_res(add, r, +1);
    }
    if (!ok) {
      Lr = j;
      c->ex_stats[4]++;
      break;
    }
    if (!any) continue;
    SampleOut& o = c->h_fix_so[j];
    o.rollouts += add.rollouts; o.steps += add.steps; o.f_col += add.f_col; o.f_acc += add.f_acc; o.f_it += add.f_it;
    patched = true;
    resolved++;
  }
  if (patched) HIPC(c, hipMemcpyAsync(c->so, c->h_fix_so.data(), sizeof(SampleOut) * Lr, hipMemcpyHostToDevice, st));
  // the verdict histogram: the committed prefix and, where the prefix ends early, the sample that ended it
  for (int j = 0; j <= Lr && j < n; j++) {
    int64_t* h = c->ex_hist;
    const int* ad = fadj + FIX_ADJ * j;
    if (fn[j] == 0) h[0]++;
    else if (fn[j] > 0 && c->h_fix_so[j].k >= 0) h[1]++;
    else if (fn[j] > 0) {
      h[2]++;
      h[3] += (ad[0] | ad[1] | ad[2] | ad[3] | ad[4]) != 0;
    } else if (fn[j] >= -4) {
      h[3 - fn[j]]++;
      if (x_fits) {  // (past the size limit such a sample ends the prefix without a recomputed list)
        h[8]++;
        h[9] += j < Lr;
        h[10] += j == not_found;
      }
    }
    h[11] += j == Lr && Lr < stop;
    h[12] += ad[5] != 0;
  }
  c->ex_stats[0]++;
  c->ex_stats[1] += resolved;
  c->ex_stats[2] += nj;
  c->ex_stats[3] += Lr < n;
  *L = std::max(1, Lr);
  return CLRRT_OK;
}

// Stages 1-4 (+5 in EXACT mode) for n samples already in cur.d_samples.  Returns the number of
// samples to commit (n in BATCH mode).  have_lists: the candidate lists are already in cur.cand
// (pipelined rounds); during_roll runs right after the rollout kernel's launch.
static int eval_samples(clrrt_ctx* c, int n, bool exact, int* L_out, bool have_lists = false,
                        const std::function<int()>& during_roll = nullptr,
                        const std::function<int()>& pre_roll = nullptr) {
  hipStream_t st = c->stream;
  ListSet& cur = *c->ls[0];
  c->totals_zeroed = false;  // (a round that failed after its prologue fill leaves nothing behind)
  KeyId* scratch = nullptr;
  if (exact) {
    int rc = ensure_sort_scratch(c, (int64_t)n * c->n_nodes);
    if (rc != CLRRT_OK) return rc;
    scratch = c->sort_scratch;
  }
  if (!have_lists) {
    int rc = run_nn(c, n, scratch);
    if (rc != CLRRT_OK) return rc;
  }
  // the tree, this round's lists and the walk buffers are final here: work queued by during_roll on
  // another stream waits for this point only, not for the rollouts
  if (pre_roll) {
    int rc = pre_roll();
    if (rc != CLRRT_OK) return rc;
  }
  if (during_roll) HIPC(c, hipEventRecord(c->ev_tree, st));
  const bool persistent = c->roll_persistent && c->dp.n_steps_max > 0;
  const bool deferred = persistent && c->rows_deferred;
  if (!deferred) {  // rows into job slots: replays pending from a deferred round run first
    int rc = flush_replays(c);
    if (rc == CLRRT_OK) rc = ensure_slots(c);
    if (rc != CLRRT_OK) return rc;
  }
  const bool defer = c->def.active && !exact && persistent && deferred;
  if (defer) {  // this round's lists and samples into its ring slot (k_select / the replays read them there)
    auto& d = c->def;
    d.slot = (int)(d.round % d.R);
    const int64_t B = c->cap.max_batch;
    HIPC(c, hipMemcpyAsync(d.cand + (int64_t)d.slot * B * CAND_K, cur.cand, sizeof(int) * n * CAND_K,
                           hipMemcpyDeviceToDevice, st));
    HIPC(c, hipMemcpyAsync(d.ncand + (int64_t)d.slot * B, cur.ncand, sizeof(int) * n, hipMemcpyDeviceToDevice, st));
    HIPC(c, hipMemcpyAsync(d.samp + (int64_t)d.slot * B, cur.d_samples, sizeof(clrrt_sample) * n,
                           hipMemcpyDeviceToDevice, st));
    if (d.nd + (int64_t)n > d.vcap) return fail(c, CLRRT_ECAPACITY, "deferred samples exceed the commit buffers");
  }
  {
    KTimer kt(c, 1, st);
    RollArgs a = roll_args(c, n * CAND_K);
    a.res = c->res_spec;
    a.res_gb = c->res_gb;
    if (defer) defer_roll_args(c, a, true);
    a.slots = deferred ? nullptr : c->slots;
    a.slot_rows = c->slot_rows;
    a.slot_jobs = (int)(c->cap.max_batch * CAND_K);
    if (deferred) {  // this launch also replays the previous commit's accepted rollouts
      a.rep = c->rep_buf;
      a.nrep = c->rep_n;
    }
    // persistent blocks (1 resident per CU: the step loop fills the register file).  The rollout kernel's
    // makespan is its longest chains, not its width, while the side stream's search of the next round
    // grows with the tree and takes the CUs the rollouts leave; so the grid narrows as the tree grows:
    // 7/8 of the CUs below 300 k nodes, 5/8 to 700 k, 1/2 to 1.1 M, 1/4 beyond (cfg3 round time by tree
    // size and width, tools/blocks_vs_size.py: each step the best or within 2% of it; a fixed 5/8 grid
    // was the best single width; the last step was 3/8 until round 8: with the queue served by length class
    // 1/4 measured +1.55% over 3/8, three runs each, and wider schedules lower, profiles/r08a_cfg3_control.txt,
    // r08a_cfg3_widths.txt).  Scheduling only: results do not depend on the width.
    const int64_t nt = c->n_nodes;
    const int eighths = nt < 300000 ? 7 : nt < 700000 ? 5 : nt < 1100000 ? 4 : 2;
    const int blocks = c->roll_blocks > 0 ? std::min(c->roll_blocks, 4 * c->n_cu)
                                          : std::max(1, (eighths * c->n_cu) / 8);
    a.coop_enable = c->roll_coop;
    a.lanes_per_wave = c->roll_lanes > 0 ? c->roll_lanes : c->roll_spread ? 0 : 64;
    if (c->roll_priority) {
      a.perm = c->roll_perm;
      a.pflag = c->roll_pflag;
      a.order_verify = c->roll_order_verify;
    }
    unsigned long long*& dbg_host = c->dbg_host;  // diagnostics heartbeat (host-mapped)
    if (c->debug_sync) {  // diagnostics: which kernel of the round does not finish
      if (!dbg_host) HIPC(c, c->mem.renew_host(&dbg_host, 8 * 4096, hipHostMallocMapped));
      memset(dbg_host, 0, sizeof(unsigned long long) * 8 * 4096);
      HIPC(c, hipHostGetDevicePointer((void**)&a.dbg, dbg_host, 0));
      HIPC(c, hipStreamSynchronize(st));
      fprintf(stderr, "[dbg] pre-rollout work done (n %d, nrep %d, ncarry %d)\n", n, a.nrep, a.ncarry);
    }
    if (persistent && defer) {
      // the round's resets in one launch: the rollout queue / carry counters and the first-success array, the
      // count of this round's samples left pending (k_select) and the compaction's totals (launch_compact)
      FillInts f;
      f.add(a.ncarry_out, 1, 0);
      f.add(c->roll_q, 1, 0);
      f.add(c->def.best + a.sbase, n, 0x7f7f7f7f);
      f.add(c->def.d_cnt + 2, 1, 0);
      f.add((int*)c->totals, 16, 0);
      HIPC(c, launch_fill_ints(st, f));
      c->totals_zeroed = true;
      HIPC(c, launch_rollout_persistent(st, a, n, c->roll_q, c->def.best, blocks, true));
    } else if (persistent)
      HIPC(c, launch_rollout_persistent(st, a, n, c->roll_q, defer ? c->def.best : c->roll_best, blocks));
    else
      HIPC(c, launch_rollout(st, SRC_SPEC, a));
    if (c->debug_sync) {
      const auto t0 = std::chrono::steady_clock::now();
      while (hipStreamQuery(st) == hipErrorNotReady) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0) {
          fprintf(stderr, "[dbg] rollout kernel not done after 10 s; waves (iterations, busy, parked, qdone|first "
                          "busy lane, j|pass, steps|chain, wp|N, t):\n");
          unsigned long long tmax = 0;
          for (int w = 0; w < 4096; w++) tmax = std::max(tmax, dbg_host[w * 8 + 7]);
          int shown = 0;
          for (int w = 0; w < 4096 && shown < 40; w++) {
            const unsigned long long* d = dbg_host + w * 8;
            if (d[7] == 0 || tmax - d[7] < 100000000ull) continue;  // still beating in the last second
            if (d[1] == 0 && d[2] == 0 && (d[3] >> 32)) continue;      // finished
            fprintf(stderr, "  wave %d: it %llu busy %016llx parked %016llx qdone %llu lane %d j %d pass %d steps %d "
                            "chain %d wp %d N %d age %.3f s\n", w, d[0], d[1], d[2], d[3] >> 32, (int)(uint32_t)d[3],
                    (int)(d[4] >> 32), (int)(uint32_t)d[4], (int)(d[5] >> 32), (int)(uint32_t)d[5], (int)(d[6] >> 32),
                    (int)(uint32_t)d[6], (double)(tmax - d[7]) * 1e-8);
            shown++;
          }
          int alive = 0;
          for (int w = 0; w < 4096; w++) alive += dbg_host[w * 8 + 7] != 0 && tmax - dbg_host[w * 8 + 7] < 100000000ull;
          fprintf(stderr, "  waves still beating: %d\n", alive);
          abort();
        }
      }
      fprintf(stderr, "[dbg] rollout kernel done: %s\n", hipGetErrorString(hipStreamQuery(st)));
    }
    if (deferred) c->rep_n = 0;
    c->eval_deferred = deferred;
  }
  if (during_roll) {  // queued behind the rollout kernel, whose persistent blocks take the CUs first
    int rc = during_roll();
    if (rc != CLRRT_OK) return rc;
  }
  SelArgs s;
  memset(&s, 0, sizeof(s));
  s.p = c->dp; s.tree = c->tree; s.cand = cur.cand; s.ckey = cur.ckey; s.ncand = cur.ncand; s.res = c->res_spec;
  s.res_gb = c->res_gb; s.regnodes = c->regnodes; s.gbnodes = c->gbnodes; s.so = c->so; s.B = n;
  if (defer) {  // views: the deferred samples of earlier rounds, then this round's
    auto& d = c->def;
    s.cand = d.cand; s.ncand = d.ncand; s.res = d.res; s.res_gb = d.res_gb;
    s.ckey = nullptr;  // the round's keys are not in the rings (EXACT's conflict threshold only)
    s.view = d.dlist[d.cur_dl];
    s.nd = d.nd;
    s.sbase = d.slot * (int)c->cap.max_batch;
    s.gv = d.gv;
    s.pend = d.pend;
    s.new_pend = d.d_cnt + 2;
    s.B = d.nd + n;  // (d_cnt[2] was reset by the round's prologue fill before the rollouts)
  }
  c->def.nd_eval = defer ? c->def.nd : -1;
  {
    KTimer kt(c, 2);
    HIPC(c, launch_select(st, s));
  }
  int L = n;
  if (exact && n > 1 && c->exact_fixup) {
    int rc = exact_fixups(c, n, &L);
    if (rc != CLRRT_OK) return rc;
  } else if (exact && n > 1) {
    c->h_int[0] = n;
    HIPC(c, hipMemcpyAsync(c->first_conflict, c->h_int, sizeof(int), hipMemcpyHostToDevice, st));
    {
      KTimer kt(c, 2);
      HIPC(c, launch_conflict(st, c->dp, n, cur.d_samples, c->regnodes, c->gbnodes, c->so, cur.ctie,
                              c->first_conflict));
    }
    HIPC(c, hipMemcpyAsync(c->h_int + 1, c->first_conflict, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPC(c, hipStreamSynchronize(st));
    L = std::max(1, std::min(n, c->h_int[1]));
  }
  *L_out = L;
  return CLRRT_OK;
}

// Stages 5-6: compact the first L samples into node records (c->out_nodes), reserve arena rows,
// copy the accepted trajectories into the arena.  *n_out = records.
static int compact_and_copy(clrrt_ctx* c, int L, int* n_out, bool merge_bbox) {
  hipStream_t st = c->stream;
  ListSet& cur = *c->ls[0];
  auto& d = c->def;
  const bool defer = d.nd_eval >= 0;  // eval_samples selected views (deferred samples + this round's)
  const int V = defer ? d.nd_eval + L : L;
  {
    KTimer kt(c, 2);
    const bool tag = defer && c->sh.fn;  // the exchange orders deferred samples by age
    HIPC(c, launch_compact(st, V, cur.d_samples, cur.cand, c->regnodes, c->gbnodes, c->so, c->n_rows, c->rank,
                           c->out_nodes, c->jobs, c->totals, c->cmp, tag ? d.slot : 0, tag ? d.R : 0,
                           (int)c->cap.max_batch, c->totals_zeroed));
    c->totals_zeroed = false;
    if (merge_bbox) HIPC(c, launch_bbox(st, c->out_nodes, c->totals, 0, c->d_bbox));
    // the views still pending, in view order: the next commit's deferred samples
    if (defer) HIPC(c, launch_defer_select(st, d.gv, d.pend, V, d.dlist[1 - d.cur_dl], d.d_cnt, d.sel_tmp, d.sel_bytes));
  }
  HIPC(c, hipMemcpyAsync(c->h_totals, c->totals, sizeof(int64_t) * 8, hipMemcpyDeviceToHost, st));
  if (merge_bbox) HIPC(c, hipMemcpyAsync(c->h_bbox, c->d_bbox, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
  if (defer) {
    HIPC(c, hipMemcpyAsync(c->h_int, d.d_cnt, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    HIPC(c, hipMemcpyAsync(c->h_int + 3, d.d_cnt + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPC(c, hipMemcpyAsync(c->h_int + 2, (const char*)(c->work_ctr + 62), sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIPC(c, hipStreamSynchronize(st));
  {
    const int rw = watchdog_check(c);
    if (rw != CLRRT_OK) return rw;
  }
  if (c->iter_log && !defer && L > 0) {  // the committed iterations' records, in sample order
    c->iter_tmp.resize(L);
    HIPC(c, hipMemcpy(c->iter_tmp.data(), c->so, sizeof(SampleOut) * L, hipMemcpyDeviceToHost));
    for (int j = 0; j < L; j++) {
      const SampleOut& o = c->iter_tmp[j];
      clrrt_iteration r;
      r.nodes = (o.k >= 0) + (o.k >= 0 && o.gb_ok);
      r.sim_count = o.steps; r.fail_collision = o.f_col; r.fail_acclimit = o.f_acc; r.fail_iterlimit = o.f_it;
      r.rollouts = o.rollouts;
      c->iters.push_back(r);
    }
  }
  if (merge_bbox) bbox_add(c, c->h_bbox[0], c->h_bbox[1], c->h_bbox[2], c->h_bbox[3]);
  if (defer) {
    if (c->h_int[2] != 0 || c->h_int[1] > d.carry_cap)
      return fail(c, CLRRT_ECAPACITY, "suspended rollouts exceed the carry buffer (raise defer_steps)");
    if (L > 0) d.deferred_total += c->h_int[3];  // this round's samples left pending (k_select)
    d.cur_dl ^= 1;
    d.nd = c->h_int[0];
    d.cur_c ^= 1;
    d.ncarry = c->h_int[1];
    d.round++;
    d.nd_eval = -1;
  }
  int64_t nn = c->h_totals[0], nr = c->h_totals[1];
  if (c->n_rows + nr > c->cap.max_rows) return fail(c, CLRRT_ECAPACITY, "trajectory arena full");
  if (c->fail_at_round > 0 && --c->fail_at_round == 0)
    return fail(c, CLRRT_ECAPACITY, "injected failure (option fail_at_round)");
  c->counters.sim_count += c->h_totals[2];
  c->counters.fail_collision += c->h_totals[3];
  c->counters.fail_acclimit += c->h_totals[4];
  c->counters.fail_iterlimit += c->h_totals[5];
  c->counters.rollouts += c->h_totals[6];
  c->last_goal_nodes = c->h_totals[7];
  if (c->eval_deferred) {  // the accepted rollouts are replayed into the arena by the next persistent launch
    if (c->rep_n > 0) {
      int rc = flush_replays(c);
      if (rc != CLRRT_OK) return rc;
    }
    KTimer kt(c, 2);
    if (defer)  // the committed samples' lists and results sit in the rings
      HIPC(c, launch_replay_gather(st, c->jobs, c->out_nodes, (int)nn, c->tree, d.cand, d.samp, d.res, c->rep_buf));
    else
      HIPC(c, launch_replay_gather(st, c->jobs, c->out_nodes, (int)nn, c->tree, cur.cand, cur.d_samples, c->res_spec,
                                   c->rep_buf));
    c->rep_n = (int)nn;
  } else {
    KTimer kt(c, 2);
    HIPC(c, launch_copy_rows(st, c->jobs, c->out_nodes, (int)nn, c->slots, c->slot_rows,
                             (int)(c->cap.max_batch * CAND_K), c->arena));
  }
  c->n_rows += nr;
  c->last_eval_rows = nr;
  *n_out = (int)nn;
  return CLRRT_OK;
}

// Deferred samples: the rings for the context's T and n_steps_max, the view-sized commit buffers and the
// carry buffers (allocated on the first expansion that defers, grown when T shrinks or sim_dt does).
static int ensure_defer(clrrt_ctx* c) {
  auto& d = c->def;
  const int64_t B = c->cap.max_batch;
  const int n = std::max(1, c->dp.n_steps_max);
  const int R = (int)((2LL * n + d.T - 1) / d.T) + 2;
  // sharded rounds carry a record's origin-round age in 8 bits (k_compact_scatter / k_xorder_keys)
  if (c->sh.fn && R > 256)
    return fail(c, CLRRT_EINVAL, "defer_steps too small for sharded rounds (more than 256 rounds in flight)");
  if (!d.res || d.R < R) {
    HIPC(c, hipStreamSynchronize(c->stream));
    d.R = 0;
    HIPC(c, c->mem.renew(&d.res, (size_t)R * B * CAND_K));
    HIPC(c, c->mem.renew(&d.res_gb, (size_t)R * B * CAND_K));
    HIPC(c, c->mem.renew(&d.cand, (size_t)R * B * CAND_K));
    HIPC(c, c->mem.renew(&d.ncand, (size_t)R * B));
    HIPC(c, c->mem.renew(&d.samp, (size_t)R * B));
    HIPC(c, c->mem.renew(&d.best, (size_t)R * B));
    d.R = R;
  }
  if (!d.gv || d.vcap < (int64_t)d.R * B) {
    // every commit path holds up to vcap views: the deferred samples (at most R - 1 earlier rounds' worth,
    // the ring) + one round
    const int64_t V = (int64_t)d.R * B;
    int rc = flush_replays(c);  // rep_buf is re-made below
    if (rc != CLRRT_OK) return rc;
    HIPC(c, hipStreamSynchronize(c->stream));
    d.vcap = 0;
    HIPC(c, c->mem.renew(&c->regnodes, V));
    HIPC(c, c->mem.renew(&c->gbnodes, V));
    HIPC(c, c->mem.renew(&c->so, V));
    HIPC(c, c->mem.renew(&c->out_nodes, 2 * V));
    HIPC(c, c->mem.renew(&c->jobs, 2 * V));
    HIPC(c, c->mem.renew_bytes(&c->rep_buf, replay_bytes() * (size_t)2 * V));
    HIPC(c, c->mem.renew(&c->cmp.packed, V));
    HIPC(c, c->mem.renew(&c->cmp.scanned, V));
    c->cmp.tmp_bytes = compact_scan_bytes((int)V);
    HIPC(c, c->mem.renew_bytes(&c->cmp.tmp, std::max<size_t>(c->cmp.tmp_bytes, 256)));
    HIPC(c, c->mem.renew(&d.dlist[0], V));
    HIPC(c, c->mem.renew(&d.dlist[1], V));
    HIPC(c, c->mem.renew(&d.gv, V));
    HIPC(c, c->mem.renew(&d.pend, V));
    d.sel_bytes = defer_select_bytes((int)V);
    HIPC(c, c->mem.renew_bytes(&d.sel_tmp, std::max<size_t>(d.sel_bytes, 256)));
    HIPC(c, c->mem.renew(&d.d_cnt, 3));
    // suspended chains: at most every job of the rounds in flight (a launch's chains all come from them)
    d.carry_cap = (int)std::min<int64_t>(V * CAND_K, 1 << 21);
    HIPC(c, c->mem.renew_bytes(&d.carry[0], carry_bytes() * (size_t)d.carry_cap));
    HIPC(c, c->mem.renew_bytes(&d.carry[1], carry_bytes() * (size_t)d.carry_cap));
    d.vcap = V;
  }
  return CLRRT_OK;
}

// The start of an expansion: deferral on for BATCH rounds when the option asks for it and the rollouts run
// persistent with deferred rows (the paths the carry records exist for).
static int defer_begin(clrrt_ctx* c, bool batch) {
  auto& d = c->def;
  d.active = batch && d.T > 0 && c->roll_persistent && c->rows_deferred && c->dp.n_steps_max > 0;
  d.nd = 0; d.ncarry = 0; d.round = 0; d.slot = 0; d.nd_eval = -1; d.deferred_total = 0;
  return d.active ? ensure_defer(c) : CLRRT_OK;
}

// Ring / carry fields of a rollout launch: this round's slot (cap T) or, for the drain (cap 0), no new jobs.
static void defer_roll_args(clrrt_ctx* c, RollArgs& a, bool capped) {
  auto& d = c->def;
  a.res = d.res;
  a.res_gb = d.res_gb;
  a.jbase = d.slot * (int)c->cap.max_batch * CAND_K;
  a.sbase = d.slot * (int)c->cap.max_batch;
  a.cap = capped ? d.T : 0;
  a.carry_in = d.carry[d.cur_c];
  a.ncarry = d.ncarry;
  a.carry_out = d.carry[1 - d.cur_c];
  a.ncarry_out = d.d_cnt + 1;
  a.carry_cap = d.carry_cap;
}

// Row slots for the paths that store speculative rows (option "rows_deferred" 0, non-persistent rollouts).
static int ensure_slots(clrrt_ctx* c) {
  const int need = c->dp.n_steps_max + 1;
  if (c->slots && c->slot_rows >= need) return CLRRT_OK;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  c->slot_rows = 0;
  HIPC(c, c->mem.renew(&c->slots, (size_t)2 * need * 10 * c->cap.max_batch * CAND_K));
  c->slot_rows = need;
  return CLRRT_OK;
}

// k_roll_run's watchdog (work counters 56..59): a wave that loops far past any correct launch exits and
// records its state; reported as an error.
static int watchdog_check(clrrt_ctx* c) {
  unsigned long long h[4];
  HIPC(c, hipMemcpy(h, c->work_ctr + 56, sizeof(h), hipMemcpyDeviceToHost));
  if (h[0] == 0) return CLRRT_OK;
  char msg[256];
  snprintf(msg, sizeof(msg), "rollout kernel watchdog: %llu waves; j %d fin %d steps %d chain %d qdone %d busy %d",
           h[0], (int)(h[1] >> 32), (int)(uint32_t)h[1], (int)(h[2] >> 32), (int)(uint32_t)h[2], (int)(h[3] >> 32),
           (int)(uint32_t)h[3]);
  return fail(c, CLRRT_EHIP, msg);
}

// Every replay must run exactly as many steps as its committed node has rows (k_roll_run counts the
// ones that do not in work counter 61 and stores no row past the node's count).  Nonzero means the
// arena's rows are not the committed rollouts': reported as an error instead of a silently wrong tree.
static int replay_check(clrrt_ctx* c) {
  HIPC(c, hipMemcpyAsync(c->h_int + 2, (const char*)(c->work_ctr + 61), sizeof(int), hipMemcpyDeviceToHost,
                         c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (c->h_int[2] != 0) return fail(c, CLRRT_EHIP, "a deferred-row replay diverged from its committed rollout");
  return watchdog_check(c);
}

// Run the pending replays (the last commit's accepted rollouts, deferred rows) on their own: before
// anything reads the arena, changes what a replay depends on (parameters, obstacles), or at the end of
// an expansion.  Same kernel, no jobs of a round.
static int flush_replays(clrrt_ctx* c) {
  auto& d = c->def;
  if (c->rep_n <= 0 && d.ncarry <= 0) return CLRRT_OK;
  HIPC(c, hipSetDevice(c->device));
  KTimer kt(c, 1);
  RollArgs a = roll_args(c, 0);
  a.res = c->res_spec;
  a.res_gb = c->res_gb;
  a.rep = c->rep_buf;
  a.nrep = c->rep_n;
  a.coop_enable = c->roll_coop;
  a.lanes_per_wave = c->roll_spread ? 0 : 64;
  // chains resumed from the carry buffer index the ring's first-success flags (ring slot x max_batch), not
  // roll_best's max_batch entries
  int* best = c->roll_best;
  if (d.ncarry > 0) {  // suspended replays of a deferring expansion: run to their end
    defer_roll_args(c, a, false);
    best = d.best;
    d.ncarry = 0;
  }
  HIPC(c, launch_rollout_persistent(c->stream, a, 0, c->roll_q, best, c->n_cu));
  c->rep_n = 0;
  return replay_check(c);
}

// The end of a deferring expansion: one launch without a cap runs every suspended chain (and replay) to its
// end, the samples still pending commit in view order (the oldest round first), then their rows replay.
static int defer_drain(clrrt_ctx* c, int64_t* goal_nodes) {
  auto& d = c->def;
  if (!d.active) return CLRRT_OK;
  const bool sharded = c->sh.fn != nullptr;  // every rank takes part in the drain's exchange
  if (d.nd > 0 || d.ncarry > 0 || sharded) {
    hipStream_t st = c->stream;
    {
      KTimer kt(c, 1);
      RollArgs a = roll_args(c, 0);
      a.rep = c->rep_buf;
      a.nrep = c->rep_n;
      a.coop_enable = c->roll_coop;
      a.lanes_per_wave = c->roll_spread ? 0 : 64;
      defer_roll_args(c, a, false);
      HIPC(c, launch_rollout_persistent(st, a, 0, c->roll_q, d.best, c->n_cu));
      c->rep_n = 0;
      d.ncarry = 0;
    }
    if (d.nd > 0 || sharded) {
      SelArgs s;
      memset(&s, 0, sizeof(s));
      s.p = c->dp; s.tree = c->tree; s.cand = d.cand; s.ckey = nullptr; s.ncand = d.ncand; s.res = d.res;
      s.res_gb = d.res_gb; s.regnodes = c->regnodes; s.gbnodes = c->gbnodes; s.so = c->so;
      s.view = d.dlist[d.cur_dl]; s.nd = d.nd; s.sbase = 0; s.gv = d.gv; s.pend = d.pend; s.B = d.nd;
      if (d.nd > 0) {
        KTimer kt(c, 2);
        HIPC(c, launch_select(st, s));
      }
      d.nd_eval = d.nd;
      int nn = 0, n_app = 0;
      int rc = compact_and_copy(c, 0, &nn, true);
      if (rc == CLRRT_OK) rc = commit_round(c, nn, c->sh.max_ms, &n_app);
      if (rc != CLRRT_OK) return rc;
      if (goal_nodes) *goal_nodes += c->last_goal_nodes;
      if (d.nd != 0 || d.ncarry != 0) return fail(c, CLRRT_EHIP, "deferred samples left after the drain");
    }
  }
  d.active = false;
  return flush_replays(c);
}

static int append_nodes(clrrt_ctx* c, const clrrt_node* dev_nodes, int n) {
  if (c->n_nodes + n > c->cap.max_nodes) return fail(c, CLRRT_ECAPACITY, "tree full");
  {
    KTimer kt(c, 2);
    HIPC(c, launch_append(c->stream, dev_nodes, n, c->n_nodes, c->tree, c->nn));
  }
  c->n_nodes += n;
  return CLRRT_OK;
}

extern "C" {

int clrrt_round_eval(clrrt_ctx* c, const clrrt_sample* samples, int32_t n, void* dev_out, int32_t* n_out) {
  if (!c || n < 0 || (n > 0 && !samples) || !n_out) return CLRRT_EINVAL;
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  if (c->n_nodes <= 0) return fail(c, CLRRT_ESTATE, "tree not initialised");
  HIPC(c, hipSetDevice(c->device));
  *n_out = 0;
  if (n == 0) return CLRRT_OK;
  // lists prefetched by the previous round (clrrt_round_prefetch) serve exactly the declared samples
  const bool have = c->pf_state == 2 && (int)c->pf_samples.size() == n &&
                    memcmp(c->pf_samples.data(), samples, sizeof(clrrt_sample) * n) == 0;
  if (!have) {
    if (c->pf_state != 0 && c->side) HIPC(c, hipStreamSynchronize(c->side));
    ListSet& cur = *c->ls[0];
    memcpy(cur.h_samples, samples, sizeof(clrrt_sample) * n);
    HIPC(c, hipMemcpyAsync(cur.d_samples, cur.h_samples, sizeof(clrrt_sample) * n, hipMemcpyHostToDevice, c->stream));
  }
  c->pf_state = 0;
  const int n2 = (int)std::min<size_t>(c->pf_next.size(), (size_t)c->cap.max_batch);
  NnSetup su{};
  bool side = false;
  if (n2 > 0 && c->nn_pipeline) {
    su = nn_setup(c);
    side = walk_serves(c, su);
  }
  auto during = [&]() -> int {
    memcpy(c->ls[1]->h_samples, c->pf_next.data(), sizeof(clrrt_sample) * n2);
    c->pf_samples.assign(c->pf_next.begin(), c->pf_next.begin() + n2);
    c->pf_state = 1;
    return launch_side_walk(c, n2, su);
  };
  c->pf_next.clear();
  int L = n, rc;
  auto build = [&]() -> int { return pre_roll_build(c, su); };
  if ((rc = eval_samples(c, n, false, &L, have, side ? std::function<int()>(during) : nullptr,
                         side ? std::function<int()>(build) : nullptr)) != CLRRT_OK)
    return rc;
  int nn = 0;
  if ((rc = compact_and_copy(c, L, &nn, false)) != CLRRT_OK) return rc;
  if (dev_out && nn > 0)
    HIPC(c, hipMemcpyAsync(dev_out, c->out_nodes, sizeof(clrrt_node) * nn, hipMemcpyDeviceToDevice, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  *n_out = nn;
  return CLRRT_OK;
}

int clrrt_round_commit(clrrt_ctx* c, const void* dev_nodes, int32_t n, int32_t local_first, int32_t local_count) {
  (void)local_first;
  (void)local_count;  // the local records' rows are only reserved by clrrt_round_eval: the next rollout
                      // launch (or clrrt_rows_flush) replays them into the arena (deferred rows)
  if (!c || n < 0 || (n > 0 && !dev_nodes)) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  const int64_t first_new = c->n_nodes;
  int rc = append_nodes(c, (const clrrt_node*)dev_nodes, n);
  if (rc != CLRRT_OK) return rc;
  if (n > 0) {
    HIPC(c, launch_bbox(c->stream, (const clrrt_node*)dev_nodes, nullptr, n, c->d_bbox));
    HIPC(c, hipMemcpyAsync(c->h_bbox, c->d_bbox, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPC(c, hipStreamSynchronize(c->stream));
  if (n > 0) bbox_add(c, c->h_bbox[0], c->h_bbox[1], c->h_bbox[2], c->h_bbox[3]);
  if (c->pf_state == 1) {  // the next round's search ran beside this round's rollouts
    // as in clrrt_expand: the appended nodes' search behind it on the side stream, the next round's
    // index into the other buffer set meanwhile
    if ((rc = side_delta_launch(c, (int)c->pf_samples.size(), first_new, n)) != CLRRT_OK) return rc;
    if (c->nnw_double && (rc = next_round_build(c)) != CLRRT_OK) return rc;
    if ((rc = side_lists_join(c)) != CLRRT_OK) return rc;
    c->pf_state = 2;
  }
  return CLRRT_OK;
}

int clrrt_rows_flush(clrrt_ctx* c) {
  if (!c) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  return flush_replays(c);
}

int clrrt_round_prefetch(clrrt_ctx* c, const clrrt_sample* next, int32_t n) {
  if (!c || n < 0 || (n > 0 && !next)) return CLRRT_EINVAL;
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  c->pf_next.assign(next, next + n);
  return CLRRT_OK;
}

// ---------------------------------------------------------------------------------------------
// Tree-partitioned search: a rank searches every sample of the round over its node range only (clrrt_nn_range), the
// ranks' lists are merged in (key, id) order (clrrt_nn_merge) and the round's rollouts run from the merged lists
// (clrrt_round_eval_lists).  The three use the context's list buffers (cand, ckey, ncand, ctie) on the main stream.
// The lists (cand, ckey, ncand) to the caller (host or device memory), after everything queued on the stream.
static int lists_out(clrrt_ctx* c, int n, int32_t* out_ids, float* out_keys, int32_t* out_n) {
  ListSet& cur = *c->ls[0];
  HIPC(c, hipMemcpyAsync(out_ids, cur.cand, sizeof(int) * CAND_K * n, hipMemcpyDefault, c->stream));
  HIPC(c, hipMemcpyAsync(out_keys, cur.ckey, sizeof(float) * CAND_K * n, hipMemcpyDefault, c->stream));
  HIPC(c, hipMemcpyAsync(out_n, cur.ncand, sizeof(int) * n, hipMemcpyDefault, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_nn_range(clrrt_ctx* c, const clrrt_sample* samples, int32_t n, int64_t first, int64_t count,
                   int32_t* out_ids, float* out_keys, int32_t* out_n) {
  if (!c || n < 0 || (n > 0 && (!samples || !out_ids || !out_keys || !out_n))) return CLRRT_EINVAL;
  if (first < 0 || count < 0 || first > c->n_nodes || count > c->n_nodes - first)
    return fail(c, CLRRT_EINVAL, "node range [" + std::to_string(first) + ", " + std::to_string(first) + " + " +
                                     std::to_string(count) + ") outside the tree's " + std::to_string(c->n_nodes) +
                                     " nodes");
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  if (n == 0) return CLRRT_OK;
  pf_discard(c);  // the list buffers are overwritten
  ListSet& cur = *c->ls[0];
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  memcpy(cur.h_samples, samples, sizeof(clrrt_sample) * n);
  HIPC(c, hipMemcpyAsync(cur.d_samples, cur.h_samples, sizeof(clrrt_sample) * n, hipMemcpyHostToDevice, st));
  c->nn_bf_keys += (int64_t)n * count;
  c->nn_samples += n;
  {
    KTimer kt(c, 0);
    HIPC(c, hipMemsetAsync(cur.ncand, 0, sizeof(int) * n, st));  // count == 0, and the brute force's empty older list
    const NnSetup su = nn_setup(c);  // the whole tree's frame: the same on every rank
    if (count > 0 && count >= c->nnw_min_nodes && su.region_ok) {
      WalkBufs& w = c->nnw_r;
      const int rc = ensure_walk_set(c, w);
      if (rc != CLRRT_OK) return rc;
      if (!c->nnr_built.matches(c->n_nodes, first, count, su, c->nnw_index, c->nnw_hscale)) {
        c->nnr_built.n = -1;
        HIPC(c, launch_nn_walk_build(st, c->nn, (int)count, su.fr, su.x0, su.y0, su.x1, su.y1, w, nullptr, (int)first));
        c->nnr_built.set(c->n_nodes, first, count, su, c->nnw_index, c->nnw_hscale);
      }
      c->nn_super_bounds += (int64_t)n * walk_super_count(count);
      KTimer kt3(c, 3);
      HIPC(c, launch_nn_walk_search(st, cur.d_samples, n, c->nn, (int)count, c->dp, su.fr, su.x0, su.y0, su.x1, su.y1, w,
                                    cur.cand, cur.ckey, cur.ncand, cur.ctie, c->work_ctr + 18, c->nnw_stateless));
    } else if (count > 0) {
      // short ranges (and trees the walk does not serve): the brute force's chunk lists over the range, caps from
      // +inf, merged into the empty list
      const int max_chunks = (int)std::max<int64_t>(1, c->partial_cap / ((int64_t)n * NN_K));
      int nch = 0;
      HIPC(c, launch_nn_delta_partial(st, cur.d_samples, n, c->nn, (int)first, (int)count, c->dp, su.fr, c->pk, c->pi,
                                      max_chunks, nullptr, nullptr, c->nn_seed, false, nullptr, &nch, c->work_ctr + 13));
      HIPC(c, launch_nn_delta_merge(st, n, nch, c->dp, c->pk, c->pi, (int)first, cur.cand, cur.ckey, cur.ncand, cur.ctie));
    }
    HIPC(c, launch_nn_lists_check(st, n, c->dp, (int)c->n_nodes, cur.cand, cur.ckey, cur.ncand, cur.ctie, nullptr));
  }
  return lists_out(c, n, out_ids, out_keys, out_n);
}

int clrrt_nn_merge(clrrt_ctx* c, int32_t n, int32_t parts, const int32_t* ids, const float* keys, const int32_t* counts,
                   int32_t* out_ids, float* out_keys, int32_t* out_n) {
  if (!c || n < 0 || parts < 1 || (n > 0 && (!ids || !keys || !counts || !out_ids || !out_keys || !out_n)))
    return CLRRT_EINVAL;
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  if (n == 0) return CLRRT_OK;
  pf_discard(c);  // the list buffers are overwritten
  ListSet& cur = *c->ls[0];
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int64_t pairs = (int64_t)parts * n;
  if (pairs > c->pm_cap) {
    HIPC(c, hipStreamSynchronize(st));
    c->pm_cap = 0;
    HIPC(c, c->mem.renew(&c->pm_ids, pairs * CAND_K));
    HIPC(c, c->mem.renew(&c->pm_keys, pairs * CAND_K));
    HIPC(c, c->mem.renew(&c->pm_counts, pairs));
    c->pm_cap = pairs;
  }
  HIPC(c, hipMemcpyAsync(c->pm_ids, ids, sizeof(int) * CAND_K * pairs, hipMemcpyDefault, st));
  HIPC(c, hipMemcpyAsync(c->pm_keys, keys, sizeof(float) * CAND_K * pairs, hipMemcpyDefault, st));
  HIPC(c, hipMemcpyAsync(c->pm_counts, counts, sizeof(int) * pairs, hipMemcpyDefault, st));
  {
    KTimer kt(c, 0);
    HIPC(c, launch_nn_merge_parts(st, n, parts, c->dp, c->pm_ids, c->pm_keys, c->pm_counts, cur.cand, cur.ckey, cur.ncand,
                                  cur.ctie));
  }
  return lists_out(c, n, out_ids, out_keys, out_n);
}

int clrrt_round_eval_lists(clrrt_ctx* c, const clrrt_sample* samples, int32_t n, const int32_t* ids, const float* keys,
                           const int32_t* counts, void* dev_out, int32_t* n_out) {
  if (!c || n < 0 || !n_out || (n > 0 && (!samples || !ids || !keys || !counts))) return CLRRT_EINVAL;
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  if (c->n_nodes <= 0) return fail(c, CLRRT_ESTATE, "tree not initialised");
  HIPC(c, hipSetDevice(c->device));
  *n_out = 0;
  if (n == 0) return CLRRT_OK;
  pf_discard(c);  // a prefetched search is for the engine's own lists
  ListSet& cur = *c->ls[0];
  hipStream_t st = c->stream;
  if (!c->d_bad) HIPC(c, c->mem.renew(&c->d_bad, 1));
  memcpy(cur.h_samples, samples, sizeof(clrrt_sample) * n);
  HIPC(c, hipMemcpyAsync(cur.d_samples, cur.h_samples, sizeof(clrrt_sample) * n, hipMemcpyHostToDevice, st));
  HIPC(c, hipMemcpyAsync(cur.cand, ids, sizeof(int) * CAND_K * n, hipMemcpyDefault, st));
  HIPC(c, hipMemcpyAsync(cur.ckey, keys, sizeof(float) * CAND_K * n, hipMemcpyDefault, st));
  HIPC(c, hipMemcpyAsync(cur.ncand, counts, sizeof(int) * n, hipMemcpyDefault, st));
  // the lists are checked on the device before any rollout reads them: counts in [0, sort_limit], listed ids inside
  // the tree (slots past the count become -1, which the rollouts skip)
  c->h_int[2] = 0x7fffffff;
  HIPC(c, hipMemcpyAsync(c->d_bad, c->h_int + 2, sizeof(int), hipMemcpyHostToDevice, st));
  HIPC(c, launch_nn_lists_check(st, n, c->dp, (int)c->n_nodes, cur.cand, cur.ckey, cur.ncand, cur.ctie, c->d_bad));
  HIPC(c, hipMemcpyAsync(c->h_int + 3, c->d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  if (c->h_int[3] != 0x7fffffff)
    return fail(c, CLRRT_EINVAL, "candidate list of sample " + std::to_string(c->h_int[3]) +
                                     ": count outside [0, sort_limit] or a node id outside the tree");
  int L = n, rc;
  if ((rc = eval_samples(c, n, false, &L, true)) != CLRRT_OK) return rc;
  int nn = 0;
  if ((rc = compact_and_copy(c, L, &nn, false)) != CLRRT_OK) return rc;
  if (dev_out && nn > 0)
    HIPC(c, hipMemcpyAsync(dev_out, c->out_nodes, sizeof(clrrt_node) * nn, hipMemcpyDeviceToDevice, st));
  HIPC(c, hipStreamSynchronize(st));
  *n_out = nn;
  return CLRRT_OK;
}

// ---------------------------------------------------------------------------------------------
// Sharded rounds: goal nodes among the records appended since the last reset (every rank's), read once at
// the end of an expansion.
static int shard_goal_reset(clrrt_ctx* c) {
  HIPC(c, hipMemsetAsync(c->sh.d_goal, 0, sizeof(unsigned long long), c->stream));
  return CLRRT_OK;
}
static int shard_goal_count(clrrt_ctx* c, int64_t* out) {
  unsigned long long v = 0;
  HIPC(c, hipMemcpyAsync(c->h_totals, c->sh.d_goal, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  memcpy(&v, c->h_totals, sizeof(v));
  *out = (int64_t)v;
  return CLRRT_OK;
}

// Sharded rounds (clrrt_set_shards): this rank's contiguous slice [f, f + n) of a round of g samples.
static inline void shard_slice(const clrrt_ctx* c, int64_t g, int64_t* f, int* n) {
  const int64_t W = c->sh.world, r = c->sh.rank;
  *f = g * r / W;
  *n = (int)(g * (r + 1) / W - *f);
}

// The end of a sharded expansion: one closing exchange on every rank (no records), which carries this rank's
// failure (aux bit 48) to the others -- a failure in its last round's post-exchange work or in the drain included,
// when no round exchange is left for them to see it in -- and reports theirs.  Skipped when every rank already
// left at the same exchange (an error flag seen there) or the collective itself failed.  Returns the final status.
static int shard_expansion_end(clrrt_ctx* c, int rc) {
  auto& h = c->sh;
  if (h.fn && !h.poison_seen && !h.fn_failed) {
    clrrt_exchange_io io;
    memset(&io, 0, sizeof(io));
    io.flags = 1;
    io.elapsed_ms = h.max_ms;
    io.aux_local = rc != CLRRT_OK ? (1ll << 48) : 0;
    io.bbox_local[0] = io.bbox_local[1] = HUGE_VAL;
    io.bbox_local[2] = io.bbox_local[3] = -HUGE_VAL;
    io.stream = (void*)c->stream;
    io.aux_sum = io.aux_local;
    const int r = h.fn(h.user, &io);
    if (rc == CLRRT_OK) {
      if (r != 0) rc = fail(c, CLRRT_EHIP, "the closing exchange of the sharded expansion failed");
      else if (io.aux_sum >> 48)
        rc = fail(c, CLRRT_EHIP, "sharded expansion: " + std::to_string(io.aux_sum >> 48) + " rank(s) failed");
    }
  }
  if (rc != CLRRT_OK) {  // the expansion's suspended chains and pending samples are dropped with its results
    c->def.ncarry = 0;
    c->def.nd = 0;
  }
  return rc;
}
static void shard_expansion_begin(clrrt_ctx* c) {
  c->sh.poison_seen = c->sh.fn_failed = false;
}

// The commit of a round's records (c->out_nodes[0 .. nn)): appended as they are (one rank), or exchanged
// with the other ranks and the union appended in the same order on every rank.  *n_app = records appended.
// Sharded, nothing here waits for the device besides the hook's read of the exchanged counts: the records go
// to dev_local on the engine's stream and the hook orders its collective after it (clrrt_exchange_io.stream);
// the ranks' position bounds travel with the counts (compact_and_copy read this rank's into h_bbox).
static int commit_round(clrrt_ctx* c, int nn, double elapsed_ms, int* n_app) {
  auto& h = c->sh;
  *n_app = 0;
  if (!h.fn) {
    *n_app = nn;
    const int rc = append_nodes(c, c->out_nodes, nn);
    if (rc == CLRRT_OK) c->round_sizes.push_back(c->n_nodes);
    return rc;
  }
  if (nn > h.cap_local) return fail(c, CLRRT_ECAPACITY, "the round's records exceed the exchange buffer");
  std::optional<KTimer> kt;
  kt.emplace(c, 5);  // the exchange's span on the engine's stream
  if (nn > 0)
    HIPC(c, hipMemcpyAsync(h.dev_local, c->out_nodes, sizeof(clrrt_node) * nn, hipMemcpyDeviceToDevice, c->stream));
  clrrt_exchange_io io;
  memset(&io, 0, sizeof(io));
  io.n_local = nn;
  io.elapsed_ms = elapsed_ms;
  // aux: this rank's pending deferred samples (low 32 bits) and whether its arena can take another round of
  // its slice (+ its deferred samples) -- summed over the ranks, so every rank takes the same stop decision
  const int64_t nd_loc = c->def.active ? c->def.nd : 0;
  const bool rows_full =
      c->n_rows + nn + 2 * ((int64_t)h.last_nb + nd_loc) * (c->dp.n_steps_max + 1) > c->cap.max_rows;
  io.aux_local = nd_loc + (rows_full ? (1ll << 32) : 0);
  for (int q = 0; q < 4; q++) io.bbox_local[q] = nn > 0 ? c->h_bbox[q] : (q < 2 ? HUGE_VAL : -HUGE_VAL);
  io.stream = (void*)c->stream;
  io.max_elapsed_ms = elapsed_ms;
  io.aux_sum = io.aux_local;
  if (h.fn(h.user, &io) != 0 || io.n_all < 0 || (io.n_all > 0 && !io.dev_all)) {
    h.fn_failed = true;
    return fail(c, CLRRT_EHIP, "the exchange of the round's records failed");
  }
  kt.reset();
  const int64_t aux_sum = io.aux_sum;
  if (aux_sum >> 48) {  // another rank failed (shard_poison): every rank leaves the expansion
    h.poison_seen = true;
    return fail(c, CLRRT_EHIP, "sharded expansion: " + std::to_string(aux_sum >> 48) + " rank(s) failed this round");
  }
  if (c->fail_after_exchange > 0 && --c->fail_after_exchange == 0)
    return fail(c, CLRRT_ECAPACITY, "injected failure (option fail_after_exchange)");
  h.max_ms = io.max_elapsed_ms;
  h.nd_global = aux_sum & 0xffffffffll;
  h.rows_stop = (aux_sum >> 32) & 0xffff;
  const int32_t n_all = io.n_all;
  void* all = io.dev_all;
  if (n_all > 0) {
    if (n_all > h.xcap) {
      HIPC(c, hipStreamSynchronize(c->stream));
      h.xcap = 0;
      const int64_t cap = std::max<int64_t>(2 * (int64_t)n_all, 4096);
      HIPC(c, c->mem.renew(&h.xbuf, cap));
      HIPC(c, c->mem.renew(&h.xkey, 4 * cap));
      h.xtmp_bytes = xorder_sort_bytes((int)cap);
      HIPC(c, c->mem.renew_bytes(&h.xtmp, std::max<size_t>(h.xtmp_bytes, 256)));
      h.xcap = cap;
    }
    HIPC(c, launch_xorder(c->stream, (const clrrt_node*)all, n_all, c->def.active, h.xkey, h.xtmp, h.xtmp_bytes,
                          h.xbuf, h.d_goal));
    int rc = append_nodes(c, h.xbuf, n_all);
    if (rc != CLRRT_OK) return rc;
    // the tree's bounding box takes every rank's records (the walk frame is then the same on every rank); the
    // union of the ranks' bounds is the bound of the union (min / max), so no pass over the gathered records
    bbox_add(c, io.bbox_all[0], io.bbox_all[1], io.bbox_all[2], io.bbox_all[3]);
  }
  *n_app = n_all;
  c->round_sizes.push_back(c->n_nodes);
  return CLRRT_OK;
}

// ---------------------------------------------------------------------------------------------
// Lag-2 pipelined BATCH rounds (option "nn_lag" 2).  BATCH rounds commit every sample, so the samples of
// the next rounds are known ahead.  The walk search of round r+2's samples runs over the tree T_r (the
// tree round r's rollouts start from) on a side stream, beside rounds r and r+1; after round r+1's
// commit the nodes those two rounds appended, [|T_r|, |T_{r+2}|), are searched and merged in
// (launch_nn_delta_merge: every appended id is larger than every older one, so the merged lists equal a search
// over T_{r+2}).  A search thus has two rounds' time instead of one.  Three list sets rotate (this
// round's, round r+1's being merged, round r+2's being searched), three walk index sets (the one being
// searched by round r+1's walk, the one by round r+2's, the one being built for the next), and two side
// streams (round r+1's merge must not wait behind round r+2's walk).  Results are those of plain rounds.
struct LagSlot {
  ListSet* set = nullptr;  // its list set (ls[1] for slot A, ls[2] for slot B)
  int n = 0;               // samples searched (0: none): this rank's slice
  int64_t g = 0;           // samples of the round (all ranks)
  int64_t tree_n = 0;      // size of the tree its walk searched
  int stream = 0;          // side stream index
};

static int lag_alloc(clrrt_ctx* c) {
  if (c->nn_order) return CLRRT_OK;
  const int64_t B = c->cap.max_batch;
  int rc = alloc_lists(c, c->sets[2], B);
  if (rc != CLRRT_OK) return rc;
  for (ListSet& s : c->sets) {
    for (hipEvent_t* e : {&s.ev, &s.evw, &s.evm})
      if (!*e) HIPC(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIPC(c, c->mem.renew(&s.wseed, B));
  }
  if (!c->side2) HIPC(c, hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
  if (!c->mst) HIPC(c, hipStreamCreateWithFlags(&c->mst, hipStreamNonBlocking));
  HIPC(c, c->mem.renew(&c->nn_order, B));  // last: marks the lag-2 members complete
  return CLRRT_OK;
}

// The appended-node walk's index set (nnw_d: the buffers launch_nn_delta_walk uses, for walk_delta_cap nodes) and,
// with nn_delta_verify, the brute force's buffers beside it.
static int alloc_walk_delta(clrrt_ctx* c) {
  WalkBufs& w = c->nnw_d;
  if (!w.P) {
    const int64_t cap = walk_delta_cap(c->cap.max_nodes, c->cap.max_batch);
    const int64_t Mp = walk_tile_count(cap) * 32;  // the padded records
    HIPC(c, c->mem.renew(&w.keys, 2 * cap));
    HIPC(c, c->mem.renew(&w.vals, cap));
    w.tmp_bytes = walk_sort_bytes((int)cap);
    HIPC(c, c->mem.renew_bytes(&w.tmp, std::max<size_t>(w.tmp_bytes, 256)));
    HIPC(c, c->mem.renew(&w.skeys, cap));
    HIPC(c, c->mem.renew(&w.sids, cap));
    HIPC(c, c->mem.renew(&w.Q, Mp));
    HIPC(c, c->mem.renew(&w.CE, Mp));
    HIPC(c, c->mem.renew(&w.ID, Mp));
    HIPC(c, c->mem.renew(&w.HEAD, Mp));
    HIPC(c, c->mem.renew(&w.trun, walk_tile_count(cap)));
    HIPC(c, c->mem.renew(&w.tiles, walk_tile_count(cap)));
    HIPC(c, c->mem.renew(&w.supers, walk_super_count(cap)));
    w.sorted_n = -1;
    w.cap_nodes = cap;
    w.cap_batch = (int)c->cap.max_batch;
    HIPC(c, c->mem.renew(&w.P, Mp));  // last: marks the set complete
  }
  w.index_kind = c->nnw_index;
  w.hscale_pct = c->nnw_hscale;
  if (c->nn_delta_verify && !c->vseed) {
    HIPC(c, c->mem.renew(&c->vpk, c->partial_cap));
    HIPC(c, c->mem.renew(&c->vpi, c->partial_cap));
    HIPC(c, c->mem.renew(&c->vseed, c->cap.max_batch));
  }
  return CLRRT_OK;
}

// Stream priorities of the lag-2 rounds (option "stream_prio"): main and merge streams highest, the walk
// streams lowest (1), or all equal (0).  Scheduling only.
static int apply_stream_prio(clrrt_ctx* c) {
  if (c->stream_prio_applied == (c->stream_prio != 0)) return CLRRT_OK;
  int lo = 0, hi = 0;
  HIPC(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
  const int p_hi = c->stream_prio ? hi : 0, p_lo = c->stream_prio ? lo : 0;
  HIPC(c, hipDeviceSynchronize());
  auto remake = [&](hipStream_t& st, int pr) -> int {
    if (st) HIPC(c, hipStreamDestroy(st));
    HIPC(c, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, pr));
    return CLRRT_OK;
  };
  int rc;
  if ((rc = remake(c->side, p_lo)) != CLRRT_OK || (rc = remake(c->side2, p_lo)) != CLRRT_OK ||
      (rc = remake(c->mst, p_hi)) != CLRRT_OK || (c->own_stream && (rc = remake(c->stream, p_hi)) != CLRRT_OK))
    return rc;
  c->stream_prio_applied = c->stream_prio != 0;
  return CLRRT_OK;
}

// ---------------------------------------------------------------------------------------------
// The skeleton of an expansion, shared by its two drivers (clrrt_expand: EXACT and lag-1 BATCH rounds; expand_lag2):
//   ExpandRun x(...);  rc = expand_begin(x, batch);
//   while (rc == CLRRT_OK && round_plan(x, ...)) rc = <the driver's round body>;
//   return expand_end(x, rc, rng, out);
// Nothing returns between expand_begin and expand_end: a round body's failure (every HIPC in it) comes back as
// its status, and the epilogue -- sharded, the closing exchange the other ranks wait in -- runs on every path.
struct ExpandRun {
  clrrt_ctx* c;
  int64_t n_iters;
  double budget_ms;
  bool sharded;
  clrrt_stats st{};
  std::chrono::steady_clock::time_point t0, tr0;  // the expansion's start, the current round's
  double ms0 = 0;                                 // query time at the current round's start
  clrrt_rng work;       // draws ahead (speculative samples)
  clrrt_rng committed;  // state after exactly `iterations` iterations
  std::deque<clrrt_sample> pending;
  int64_t nodes_before;
  double last_round_ms = 0;
  ExpandRun(clrrt_ctx* c_, const clrrt_rng& rng, int64_t n_iters_, double budget_ms_)
      : c(c_), n_iters(n_iters_), budget_ms(budget_ms_), sharded(c_->sh.fn != nullptr),
        t0(std::chrono::steady_clock::now()), tr0(t0), work(rng), committed(rng), nodes_before(c_->n_nodes) {}
  double ms_since(std::chrono::steady_clock::time_point t) const {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  }
};

// The status goes into the driver's loop condition, never out of the driver.
static int expand_begin(ExpandRun& x, bool batch) {
  clrrt_ctx* c = x.c;
  c->sh.max_ms = 0;
  c->sh.nd_global = 0;
  c->sh.rows_stop = 0;
  c->totals_zeroed = false;
  shard_expansion_begin(c);
  int rc = defer_begin(c, batch);
  if (rc == CLRRT_OK && x.sharded) rc = shard_goal_reset(c);
  return rc;
}

static void draw_to(ExpandRun& x, int64_t want) {
  while ((int64_t)x.pending.size() < want) {
    clrrt_sample smp;
    clrrt_draw_samples(&x.c->params, &x.work, 1, &smp);
    x.pending.push_back(smp);
  }
}

// Whether another round of up to `cur` samples runs: false when the iterations or the budget are used up, and when
// the capacity cannot take the round -- st.capacity_stop for a budget query, *rc = CLRRT_ECAPACITY for an iteration
// count.  *gb: the round's samples over all ranks; this rank's slice is [*f0, *f0 + *nb).
static bool round_plan(ExpandRun& x, int64_t cur, int* rc, int64_t* gb, int64_t* f0, int* nb) {
  clrrt_ctx* c = x.c;
  x.tr0 = std::chrono::steady_clock::now();
  if (x.n_iters > 0 && x.st.iterations >= x.n_iters) return false;
  x.ms0 = std::chrono::duration<double, std::milli>(x.tr0 - x.t0).count();
  // sharded: every rank decides on the largest elapsed time over the ranks (the same rounds everywhere)
  if (x.n_iters == 0 && !((x.sharded ? c->sh.max_ms : x.ms0) < x.budget_ms)) return false;
  *gb = x.n_iters > 0 ? std::min<int64_t>(cur, x.n_iters - x.st.iterations) : cur;
  *f0 = 0;
  *nb = (int)*gb;
  if (x.sharded) shard_slice(c, *gb, f0, nb);
  c->sh.last_nb = *nb;
  // a round appends at most 2 nodes and 2 full-horizon trajectories per sample (+ the deferred samples that
  // resolve; sharded, the same decision on every rank: node counts only, deferred samples bounded by the ring)
  const int64_t nc = *gb + (x.sharded ? c->sh.nd_global : (int64_t)c->def.nd);
  if (c->n_nodes + 2 * nc > c->cap.max_nodes ||
      (x.sharded ? c->sh.rows_stop > 0 : c->n_rows + 2 * nc * (c->dp.n_steps_max + 1) > c->cap.max_rows)) {
    if (x.n_iters > 0) *rc = fail(c, CLRRT_ECAPACITY, "tree capacity exhausted");
    else x.st.capacity_stop = 1;
    return false;
  }
  return true;
}

// A committed round: `used` iterations consumed (three draws each), `speculated` samples evaluated.
static void round_done(ExpandRun& x, int64_t used, int64_t speculated) {
  for (int64_t j = 0; j < used; j++) {
    x.pending.pop_front();
    for (int q = 0; q < 3; q++) clrrt_rng_next(&x.committed);
  }
  x.st.iterations += used;
  x.st.goal_nodes_added += x.c->last_goal_nodes;
  x.st.speculated += speculated;
  x.st.rounds++;
  x.last_round_ms = x.ms_since(x.tr0);
}

// The end of an expansion, on every path out of its rounds.
static int expand_end(ExpandRun& x, int rc, clrrt_rng* rng, clrrt_stats* out) {
  clrrt_ctx* c = x.c;
  // the deferred samples still pending (sharded: an exchange the other ranks expect) and the last round's accepted
  // rows: part of the query's output tree, so inside its time
  if (rc == CLRRT_OK) rc = defer_drain(c, &x.st.goal_nodes_added);
  x.st.deferred = c->def.deferred_total;
  if (rc == CLRRT_OK) {
    rc = flush_replays(c);
  } else if (rc == CLRRT_ECAPACITY) {
    // A refused round (or one that failed on a capacity) leaves rows of committed nodes owed: the last commit's
    // replays and, with deferred samples, the replays the cap suspended -- they sit in the carry buffer beside the
    // abandoned samples' chains, which shard_expansion_end and the next defer_begin forget.  They run to their end
    // now (the abandoned chains with them; nothing selects their results).  The refusal stays the error.
    const std::string err = c->err;
    (void)flush_replays(c);
    c->err = err;
  }
  if (rc == CLRRT_OK && x.sharded) rc = shard_goal_count(c, &x.st.goal_nodes_added);
  // every stream drained, the first error kept: before the closing exchange, so a late asynchronous error travels in it
  for (hipStream_t s : {c->side, c->side2, c->mst, c->stream}) {
    const hipError_t e = s ? hipStreamSynchronize(s) : hipSuccess;
    if (e != hipSuccess && rc == CLRRT_OK)
      rc = fail(c, CLRRT_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  }
  rc = shard_expansion_end(c, rc);  // the closing exchange (sharded): every rank learns of any rank's failure
  c->def.active = false;
  // the walk sets' kept indexes and sort results were built by this expansion's schedule: the next user rebuilds
  c->nnw_built.n = -1;
  c->nnw.sorted_n = c->nnw_alt.sorted_n = c->nnw3.sorted_n = -1;
  x.st.nodes_added = c->n_nodes - x.nodes_before;
  x.st.elapsed_ms = x.ms_since(x.t0);
  *rng = x.committed;
  if (out) *out = x.st;
  return rc;
}

static int expand_lag2(clrrt_ctx* c, clrrt_rng* rng, int64_t n_iters, double budget_ms, int32_t batch,
                       clrrt_stats* out) {
  int rc = lag_alloc(c);
  if (rc == CLRRT_OK && c->nn_delta_walk) rc = alloc_walk_delta(c);
  if (rc == CLRRT_OK) rc = apply_stream_prio(c);
  if (rc != CLRRT_OK) return rc;
  ExpandRun x(c, *rng, n_iters, budget_ms);
  rc = expand_begin(x, true);
  const int cur = batch;  // samples per round, all ranks
  const bool sharded = x.sharded;
  hipStream_t sides[2] = {c->side, c->side2};
  WalkBufs* W[3] = {&c->nnw, &c->nnw_alt, &c->nnw3};
  BuiltFor built[3];  // what each walk set's index was built for
  // list sets: this round's (ls[0]), round r+1's (slot A: ls[1]) and round r+2's (slot B: ls[2])
  LagSlot A, B;
  A.set = c->ls[1];
  B.set = c->ls[2];
  // The appended-node search walks its range's own index (nn_delta_walk) from one tile of appended nodes on: a range
  // inside one tile has a single bound, so the walk would prefilter every record as k_nn_partial does, behind three
  // more launches (a range above the set's capacity takes the brute force too).
  const int64_t delta_walk_min = 32;
  const bool delta_walk = c->nn_delta_walk != 0;
  bool have_cur = false;  // this round's lists come from slot A of the previous round
  int cur_stream = 0;
  // the index of the tree as it is now into walk set k (incremental from the set built before, if any)
  auto build = [&](int k, const NnSetup& su) -> int {
    if (tree_index_matches(c, built[k], su)) return CLRRT_OK;
    int r2 = ensure_walk_set(c, *W[k]);
    if (r2 != CLRRT_OK) return r2;
    const WalkBufs* prev = nullptr;
    for (int q = 1; q <= 2 && !prev; q++) {
      const WalkBufs* w = W[(k + 3 - q) % 3];
      if (w->P && w->sorted_n > 0) prev = w;
    }
    KTimer kt(c, 0, c->stream);
    HIPC(c, launch_nn_walk_build(c->stream, c->nn, (int)c->n_nodes, su.fr, su.x0, su.y0, su.x1, su.y1, *W[k], prev));
    tree_index_set(c, built[k], su);
    return CLRRT_OK;
  };
  // slot sl: the walk search of its n samples (its set's host copy) over the current tree (walk set k)
  auto walk = [&](LagSlot& sl, int n, int k, const NnSetup& su, int si) -> int {
    hipStream_t s = sides[si];
    ListSet& l = *sl.set;
    int r2 = ensure_walk_set(c, *W[k]);  // the configuration (budgets) for this tree size
    if (r2 != CLRRT_OK) return r2;
    c->nn_bf_keys += (int64_t)n * c->n_nodes;
    c->nn_samples += n;
    HIPC(c, hipStreamWaitEvent(s, c->ev_tree, 0));
    HIPC(c, hipMemcpyAsync(l.d_samples, l.h_samples, sizeof(clrrt_sample) * n, hipMemcpyHostToDevice, s));
    c->nn_super_bounds += (int64_t)n * walk_super_count(c->n_nodes);
    {
      KTimer kt(c, 0, s), kt3(c, 3, s);
      W[k]->seed_out = l.wseed;
      W[k]->ev_main = l.evm;
      const hipError_t ew = launch_nn_walk_search(s, l.d_samples, n, c->nn, (int)c->n_nodes, c->dp, su.fr, su.x0, su.y0,
                                                  su.x1, su.y1, *W[k], l.cand, l.ckey, l.ncand, l.ctie, c->work_ctr + 18,
                                                  c->nnw_stateless);
      W[k]->seed_out = nullptr;
      W[k]->ev_main = nullptr;
      HIPC(c, ew);
    }
    HIPC(c, hipEventRecord(l.evw, s));
    sl.n = n;
    sl.tree_n = c->n_nodes;
    sl.stream = si;
    return CLRRT_OK;
  };
  // round k: gb samples over all ranks, this rank's slice [f0, f0 + nb)
  auto round = [&](int64_t k, int64_t gb, int64_t f0, int nb) -> int {
    int r = CLRRT_OK;
    auto& pending = x.pending;
    ListSet& cs = *c->ls[0];
    const int64_t left = n_iters > 0 ? n_iters - x.st.iterations : INT64_MAX;
    const double ms0 = x.ms0;
    const int wk = (int)(k % 3);
    const NnSetup su = nn_setup(c);
    const bool serve = c->n_nodes >= c->nnw_min_nodes && su.region_ok;
    // samples of rounds r+1 (slot A, unless already searched) and r+2 (slot B) to search this round (gA, gB
    // over all ranks; nA, nB this rank's slices)
    int64_t gA = 0, gB = 0, fA = 0, fB = 0;
    int nA = 0, nB = 0;
    if (serve) {
      const bool more = n_iters > 0 || ms0 + 2.0 * x.last_round_ms < budget_ms;
      if (A.n == 0 && (n_iters > 0 || ms0 + x.last_round_ms < budget_ms)) gA = std::max<int64_t>(0, std::min<int64_t>(cur, left - gb));
      const int64_t gA_eff = A.n > 0 ? A.g : gA;
      if (more && gA_eff > 0) gB = std::max<int64_t>(0, std::min<int64_t>(cur, left - gb - gA_eff));
      nA = (int)gA;
      nB = (int)gB;
      if (sharded) {
        shard_slice(c, gA, &fA, &nA);
        shard_slice(c, gB, &fB, &nB);
      }
    }
    const int64_t gA_all = A.n > 0 ? A.g : gA;
    draw_to(x, gb + gA_all + gB);
    // this round's lists
    if (have_cur) {
      KTimer kt(c, 4);  // the lists' wait (time the main stream stalls on the side streams)
      HIPC(c, hipStreamWaitEvent(c->stream, cs.ev, 0));
    } else {
      for (int j = 0; j < nb; j++) cs.h_samples[j] = pending[f0 + j];
      HIPC(c, hipMemcpyAsync(cs.d_samples, cs.h_samples, sizeof(clrrt_sample) * nb, hipMemcpyHostToDevice, c->stream));
      if (serve) {
        // the side streams' work is done (a first pipelined round searches nothing ahead yet)
        HIPC(c, hipStreamSynchronize(c->side));
        HIPC(c, hipStreamSynchronize(c->side2));
        HIPC(c, hipStreamSynchronize(c->mst));
        if ((r = build(wk, su)) != CLRRT_OK) return r;
        c->nn_bf_keys += (int64_t)nb * c->n_nodes;
        c->nn_samples += nb;
        c->nn_super_bounds += (int64_t)nb * walk_super_count(c->n_nodes);
        KTimer kt(c, 0), kt3(c, 3);
        HIPC(c, launch_nn_walk_search(c->stream, cs.d_samples, nb, c->nn, (int)c->n_nodes, c->dp, su.fr, su.x0, su.y0,
                                      su.x1, su.y1, *W[wk], cs.cand, cs.ckey, cs.ncand, cs.ctie, c->work_ctr + 18,
                                      c->nnw_stateless));
      } else if ((r = run_nn(c, nb, nullptr)) != CLRRT_OK) {
        return r;
      }
    }
    if (serve && (nA > 0 || nB > 0) && (r = build(wk, su)) != CLRRT_OK) return r;
    // searches ahead, beside this round's rollouts: slot A's (bootstrap) then slot B's; B on the other
    // side stream than A, except when both search this round's index (the walk set's sample scratch
    // is shared: one stream)
    auto ahead = [&]() -> int {
      if (nA > 0) {
        for (int j = 0; j < nA; j++) A.set->h_samples[j] = pending[gb + fA + j];
        const int r2 = walk(A, nA, wk, su, cur_stream);
        if (r2 != CLRRT_OK) return r2;
        A.g = gA;
      }
      if (nB > 0) {
        for (int j = 0; j < nB; j++) B.set->h_samples[j] = pending[gb + gA_all + fB + j];
        const int r2 = walk(B, nB, wk, su, nA > 0 ? A.stream : 1 - A.stream);
        if (r2 != CLRRT_OK) return r2;
        B.g = gB;
      }
      return CLRRT_OK;
    };
    int L = nb, nn = 0, n_app = 0;
    if ((r = eval_samples(c, nb, false, &L, true, (nA > 0 || nB > 0) ? std::function<int()>(ahead) : nullptr,
                          nullptr)) != CLRRT_OK)
      return r;
    if ((r = compact_and_copy(c, L, &nn, true)) != CLRRT_OK) return r;
    if ((r = commit_round(c, nn, x.ms_since(x.t0), &n_app)) != CLRRT_OK) return r;
    if (c->fail_in_round > 0 && --c->fail_in_round == 0)
      return fail(c, CLRRT_ECAPACITY, "injected failure (option fail_in_round)");
    // slot A: merge the nodes appended since its walk's tree.  On the merge stream, behind the commit and slot A's main
    // walk grid (caps from its k_walk_seed, beside the walk's overflow split); the merge behind the whole walk.  The
    // search walks the range's own index (launch_nn_delta_walk) where the walk is served (region, tree size) and the
    // range is neither tiny nor beyond the set; else the brute force.
    if (A.n > 0) {
      ListSet& a = *A.set;
      HIPC(c, hipEventRecord(c->ev_commit, c->stream));
      hipStream_t s = c->mst;
      HIPC(c, hipStreamWaitEvent(s, c->ev_commit, 0));
      HIPC(c, hipStreamWaitEvent(s, a.evm, 0));
      const int64_t first = A.tree_n, cnt = c->n_nodes - A.tree_n;
      const NnSetup su2 = nn_setup(c);
      const bool dwalk = delta_walk && su2.region_ok && c->n_nodes >= c->nnw_min_nodes && cnt >= delta_walk_min &&
                         cnt <= c->nnw_d.cap_nodes;
      const int max_chunks = (int)std::max<int64_t>(1, c->partial_cap / ((int64_t)A.n * NN_K));
      int nch = 0, id0 = (int)first;
      if (cnt > 0) c->nn_bf_keys += (int64_t)A.n * cnt;
      if (cnt > 0 && dwalk) {
        KTimer kt(c, 0, s);
        const bool verify = c->nn_delta_verify && c->vseed;
        HIPC(c, launch_nn_delta_walk(s, a.d_samples, A.n, c->nn, (int)first, (int)cnt, c->dp, su2.fr, su2.x0, su2.y0,
                                     su2.x1, su2.y1, c->nnw_d, c->pk, c->pi, a.wseed,
                                     verify ? c->work_ctr + 40 : nullptr));
        nch = 1;
        id0 = 0;
        if (verify) {  // the brute force over the same range and caps, and the two list sets compared
          int vch = 0;
          HIPC(c, hipMemcpyAsync(c->vseed, a.wseed, sizeof(float) * A.n, hipMemcpyDeviceToDevice, s));
          HIPC(c, launch_nn_delta_partial(s, a.d_samples, A.n, c->nn, (int)first, (int)cnt, c->dp, su2.fr, c->vpk,
                                          c->vpi, max_chunks, nullptr, nullptr, c->vseed, true, nullptr, &vch,
                                          c->work_ctr + 52));
          HIPC(c, launch_nn_delta_compare(s, A.n, vch, (int)first, c->vpk, c->vpi, c->pk, c->pi, c->work_ctr + 38));
        }
      } else if (cnt > 0) {
        KTimer kt(c, 0, s);
        HIPC(c, launch_nn_delta_partial(s, a.d_samples, A.n, c->nn, (int)first, (int)cnt, c->dp, su2.fr, c->pk, c->pi,
                                        max_chunks, nullptr, nullptr, a.wseed, true, c->nn_order, &nch));
      }
      HIPC(c, hipStreamWaitEvent(s, a.evw, 0));
      if (nch > 0) {
        KTimer kt(c, 0, s);
        HIPC(c, launch_nn_delta_merge(s, A.n, nch, c->dp, c->pk, c->pi, id0, a.cand, a.ckey, a.ncand, a.ctie));
      }
      HIPC(c, hipEventRecord(a.ev, s));
    }
    // the next round's index (the walk of round r+3's samples searches it)
    {
      const NnSetup sn = nn_setup(c);
      if (B.n > 0 && c->n_nodes >= c->nnw_min_nodes && sn.region_ok && (r = build((int)((k + 1) % 3), sn)) != CLRRT_OK)
        return r;
    }
    round_done(x, gb, gb);
    // rotate: slot A's set becomes this round's, slot B becomes slot A, this round's set serves the new slot B
    have_cur = A.n > 0;
    cur_stream = A.stream;
    std::rotate(c->ls, c->ls + 1, c->ls + 3);
    A = B;
    B = LagSlot{};
    B.set = c->ls[2];
    B.stream = 1 - A.stream;
    return CLRRT_OK;
  };
  int64_t gb = 0, f0 = 0;
  int nb = 0;
  for (int64_t k = 0; rc == CLRRT_OK && round_plan(x, cur, &rc, &gb, &f0, &nb); k++) rc = round(k, gb, f0, nb);
  return expand_end(x, rc, rng, out);
}

int clrrt_expand(clrrt_ctx* c, clrrt_rng* rng, int64_t n_iters, double budget_ms, int32_t mode, int32_t batch,
                 clrrt_stats* out) {
  if (!c || !rng || n_iters < 0 || (mode != CLRRT_MODE_EXACT && mode != CLRRT_MODE_BATCH)) return CLRRT_EINVAL;
  pf_reset(c);
  if (n_iters == 0 && !(budget_ms > 0)) return CLRRT_EINVAL;
  if (c->n_nodes <= 0) return fail(c, CLRRT_ESTATE, "tree not initialised");
  c->round_sizes.clear();
  const bool sharded = c->sh.fn != nullptr;
  if (sharded && mode != CLRRT_MODE_BATCH) return fail(c, CLRRT_EINVAL, "sharded expansion runs BATCH rounds only");
  HIPC(c, hipSetDevice(c->device));
  // samples per round (all ranks when sharded: each rank's slice must fit max_batch)
  const int64_t bmax = (int64_t)c->cap.max_batch * c->sh.world;
  batch = (int32_t)std::max<int64_t>(1, std::min<int64_t>(batch > 0 ? batch : bmax, bmax));
  if (sharded && batch < c->sh.world) return fail(c, CLRRT_EINVAL, "fewer samples per round than ranks");
  const int lag = c->nn_lag ? c->nn_lag
                  : (n_iters == 0 ? budget_ms >= 1000.0 : n_iters >= 64 * (int64_t)batch) ? 2 : 1;
  if (mode == CLRRT_MODE_BATCH && c->nn_pipeline && lag == 2) return expand_lag2(c, rng, n_iters, budget_ms, batch, out);
  ExpandRun x(c, *rng, n_iters, budget_ms);
  const bool exact = mode == CLRRT_MODE_EXACT;
  int cur = exact ? std::min(batch, std::max(16, c->exact_min_width)) : batch;
  int rc = expand_begin(x, !exact);
  bool have_next = false;  // this round's samples and lists were prepared by the previous round
  // one round: gb samples over all ranks, this rank's slice [f0, f0 + nb)
  auto round = [&](int64_t gb, int64_t f0, int nb) -> int {
    int r = CLRRT_OK;
    auto& pending = x.pending;
    const auto& st = x.st;
    draw_to(x, gb);
    if (!have_next) {
      ListSet& cs = *c->ls[0];
      for (int j = 0; j < nb; j++) cs.h_samples[j] = pending[f0 + j];
      HIPC(c, hipMemcpyAsync(cs.d_samples, cs.h_samples, sizeof(clrrt_sample) * nb, hipMemcpyHostToDevice, c->stream));
    }
    // Pipelined BATCH rounds: the next round's samples are known now (BATCH rounds commit every
    // sample), so their walk search over this round's tree runs on the side stream while this round's
    // rollouts run (the rollout kernel's last waves leave most CUs idle); after the commit, the nodes
    // this round appended are searched and merged in (launch_nn_delta).  The lists equal a search over
    // the committed tree, so the rounds' results are unchanged.
    int64_t gb2 = 0, f2 = 0;
    int nb2 = 0;
    NnSetup su{};
    if (!exact && c->nn_pipeline) {
      gb2 = cur;
      if (n_iters > 0) gb2 = std::max<int64_t>(0, std::min<int64_t>(gb2, n_iters - st.iterations - gb));
      if (n_iters == 0 && !(x.ms_since(x.t0) + x.last_round_ms < budget_ms)) gb2 = 0;  // this is probably the last round
      nb2 = (int)gb2;
      if (sharded) shard_slice(c, gb2, &f2, &nb2);
      if (nb2 > 0) {
        su = nn_setup(c);
        if (!walk_serves(c, su)) nb2 = 0;
      }
    }
    auto prefetch = [&]() -> int {
      draw_to(x, gb + gb2);
      for (int j = 0; j < nb2; j++) c->ls[1]->h_samples[j] = pending[gb + f2 + j];
      return launch_side_walk(c, nb2, su);
    };
    int L = nb, nn = 0, n_app = 0;
    auto build = [&]() -> int { return pre_roll_build(c, su); };
    if ((r = eval_samples(c, nb, exact, &L, have_next, nb2 > 0 ? std::function<int()>(prefetch) : nullptr,
                          nb2 > 0 ? std::function<int()>(build) : nullptr)) != CLRRT_OK)
      return r;
    if (!exact) {
      // BATCH rounds commit every sample, so the next round's samples are known now: draw them
      // while the GPU evaluates this round (the draw is ~0.05 us per sample on the host)
      int64_t want = gb + (int64_t)cur;
      if (n_iters > 0) want = std::min<int64_t>(want, n_iters - st.iterations);
      draw_to(x, want);
    }
    if ((r = compact_and_copy(c, L, &nn, true)) != CLRRT_OK) return r;
    const int64_t first_new = c->n_nodes;
    if ((r = commit_round(c, nn, x.ms_since(x.t0), &n_app)) != CLRRT_OK) return r;
    if (c->fail_in_round > 0 && --c->fail_in_round == 0)
      return fail(c, CLRRT_ECAPACITY, "injected failure (option fail_in_round)");
    have_next = false;
    if (nb2 > 0) {
      if ((r = side_delta_launch(c, nb2, first_new, n_app)) != CLRRT_OK) return r;
      if (c->nnw_double && (r = next_round_build(c)) != CLRRT_OK) return r;
      if ((r = side_lists_join(c)) != CLRRT_OK) return r;
      have_next = true;
    }
    // iterations consumed: the committed prefix (EXACT) or the whole round (BATCH, every rank's samples)
    round_done(x, exact ? L : gb, exact ? nb : gb);
    if (exact) cur = std::max(c->exact_min_width, std::min(batch, L == nb ? 2 * nb : 2 * L));
    return CLRRT_OK;
  };
  int64_t gb = 0, f0 = 0;
  int nb = 0;
  while (rc == CLRRT_OK && round_plan(x, cur, &rc, &gb, &f0, &nb)) rc = round(gb, f0, nb);
  return expand_end(x, rc, rng, out);
}

int clrrt_set_shards(clrrt_ctx* c, int32_t rank, int32_t world, void* dev_local, int32_t cap_local,
                     clrrt_exchange_fn exchange, void* user) {
  if (!c || world < 1 || rank < 0 || rank >= world) return CLRRT_EINVAL;
  // one rank keeps the hook only with option "shard_hook_world1" (and a hook to keep)
  const bool on = world > 1 || (c->sh.hook_world1 && exchange != nullptr);
  if (on && (!dev_local || cap_local <= 0 || !exchange)) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  auto& h = c->sh;
  h.rank = rank;
  h.world = world;
  h.dev_local = on ? dev_local : nullptr;
  h.cap_local = on ? cap_local : 0;
  h.fn = on ? exchange : nullptr;
  h.user = on ? user : nullptr;
  c->rank = rank;  // owner of this rank's records
  if (on && !h.d_goal) HIPC(c, c->mem.renew(&h.d_goal, 1));
  return CLRRT_OK;
}

int clrrt_rollout_batch(clrrt_ctx* c, const clrrt_rollout_job* jobs, int32_t n, clrrt_rollout_result* out,
                        double* rows_out, int32_t rows_cap) {
  if (!c || n < 0 || (n > 0 && (!jobs || !out))) return CLRRT_EINVAL;
  pf_reset(c);
  if (rows_out && rows_cap < c->dp.n_steps_max + 1) return fail(c, CLRRT_EINVAL, "rows_cap < max steps + 1");
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  for (int j = 0; j < n; j++)
    if (jobs[j].parent < 0 || jobs[j].parent >= c->n_nodes) return fail(c, CLRRT_EINVAL, "job parent out of range");
  std::vector<Job> hj(n);
  for (int j = 0; j < n; j++) {
    hj[j].parent = jobs[j].parent; hj[j].from_reg = 0; hj[j].gb = jobs[j].gb; hj[j].pad = 0;
    hj[j].sx = jobs[j].sample[0]; hj[j].sy = jobs[j].sample[1];
    hj[j].row_off = rows_out ? (int64_t)j * rows_cap : -1;
  }
  const char* const pre = "rollout_batch: ";
  std::vector<RollRes> hr(n);  // (before the scratch: outlives its frees, which drain the copies into it)
  Scratch<Job> dj;
  Scratch<RollRes> dr;
  Scratch<double> drows;
  HIPP(c, pre, dj.alloc(n));
  HIPP(c, pre, dr.alloc(n));
  if (rows_out) HIPP(c, pre, drows.alloc(10 * (size_t)rows_cap * n));
  HIPP(c, pre, hipMemcpyAsync(dj, hj.data(), sizeof(Job) * n, hipMemcpyHostToDevice, c->stream));
  {
    RollArgs a = roll_args(c, n);
    a.jobs = dj;
    a.arena = drows;
    a.res = dr;
    KTimer kt(c, 1);
    HIPP(c, pre, launch_rollout(c->stream, SRC_LIST, a));
  }
  HIPP(c, pre, hipMemcpyAsync(hr.data(), dr, sizeof(RollRes) * n, hipMemcpyDeviceToHost, c->stream));
  if (rows_out)
    HIPP(c, pre, hipMemcpyAsync(rows_out, drows, sizeof(double) * 10 * (size_t)rows_cap * n, hipMemcpyDeviceToHost,
                                c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  for (int j = 0; j < n; j++) {
    clrrt_rollout_result& o = out[j];
    memset(&o, 0, sizeof(o));
    o.outcome = hr[j].outcome;
    o.nrows = hr[j].nrows;
    o.costE = hr[j].costE;
    o.costS = hr[j].costS;
    for (int k = 0; k < 10; k++) o.final_state[k] = hr[j].st[k];
    o.ref_back[0] = hr[j].bx; o.ref_back[1] = hr[j].by;
    o.ref_vback = hr[j].vback;
    o.ref_n = hr[j].refN;
  }
  return CLRRT_OK;
}

int clrrt_simulate(clrrt_ctx* c, const clrrt_sim_case* cases, int32_t n, clrrt_rollout_result* out, double* rows_out,
                   int32_t rows_cap, double* ref_out, int32_t ref_cap) {
  if (!c || n < 0 || (n > 0 && (!cases || !out)) || (ref_out && ref_cap <= 0)) return CLRRT_EINVAL;
  pf_reset(c);
  if (rows_out && rows_cap < c->dp.n_steps_max + 1) return fail(c, CLRRT_EINVAL, "rows_cap < max steps + 1");
  for (int j = 0; j < n; j++)
    if (!cases[j].goal_biased && cases[j].ref_n < 1) return fail(c, CLRRT_EINVAL, "ref_n < 1");
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  std::vector<SimJob> hj(n);
  for (int j = 0; j < n; j++) {
    const clrrt_sim_case& q = cases[j];
    SimJob& s = hj[j];
    for (int k = 0; k < 10; k++) s.st[k] = q.state[k];
    s.ax = q.ax; s.ay = q.ay; s.hx = q.hx; s.hy = q.hy; s.vstart = q.vstart;
    s.n = q.ref_n; s.gb = q.goal_biased ? 1 : 0;
    s.row_off = rows_out ? (int64_t)j * rows_cap : -1;
    s.ref_off = ref_out ? (int64_t)j * 3 * ref_cap : -1;
  }
  const char* const pre = "simulate: ";
  std::vector<RollRes> hr(n);  // (before the scratch: outlives its frees, which drain the copies into it)
  Scratch<SimJob> dj;
  Scratch<RollRes> dr;
  Scratch<double> drows, dref;
  HIPP(c, pre, dj.alloc(n));
  HIPP(c, pre, dr.alloc(n));
  if (rows_out) HIPP(c, pre, drows.alloc(10 * (size_t)rows_cap * n));
  if (ref_out) HIPP(c, pre, dref.alloc(3 * (size_t)ref_cap * n));
  HIPP(c, pre, hipMemcpyAsync(dj, hj.data(), sizeof(SimJob) * n, hipMemcpyHostToDevice, c->stream));
  {
    RollArgs a = roll_args(c, n);
    a.sims = dj;
    a.arena = drows;
    a.refv = dref;
    a.ref_cap = ref_cap;
    a.res = dr;
    KTimer kt(c, 1);
    HIPP(c, pre, launch_rollout(c->stream, SRC_EXPL, a));
  }
  HIPP(c, pre, hipMemcpyAsync(hr.data(), dr, sizeof(RollRes) * n, hipMemcpyDeviceToHost, c->stream));
  if (rows_out)
    HIPP(c, pre, hipMemcpyAsync(rows_out, drows, sizeof(double) * 10 * (size_t)rows_cap * n, hipMemcpyDeviceToHost,
                                c->stream));
  if (ref_out)
    HIPP(c, pre, hipMemcpyAsync(ref_out, dref, sizeof(double) * 3 * (size_t)ref_cap * n, hipMemcpyDeviceToHost,
                                c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  for (int j = 0; j < n; j++) {
    clrrt_rollout_result& o = out[j];
    memset(&o, 0, sizeof(o));
    o.outcome = hr[j].outcome;
    o.nrows = hr[j].nrows;
    o.costE = hr[j].costE;
    o.costS = hr[j].costS;
    for (int k = 0; k < 10; k++) o.final_state[k] = hr[j].st[k];
    o.ref_back[0] = hr[j].bx; o.ref_back[1] = hr[j].by;
    o.ref_vback = hr[j].vback;
    o.ref_n = hr[j].refN;
  }
  return CLRRT_OK;
}

int clrrt_selftest_math(clrrt_ctx* c, int32_t fn, const double* a, const double* b, int32_t n, double* out) {
  if (!c || n < 0 || (n > 0 && (!a || !b || !out)) || fn < 0 || fn > 29) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const char* const pre = "selftest_math: ";
  Scratch<double> da, db, dout;
  HIPP(c, pre, da.alloc(n));
  HIPP(c, pre, db.alloc(n));
  HIPP(c, pre, dout.alloc(n));
  HIPP(c, pre, hipMemcpyAsync(da, a, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, hipMemcpyAsync(db, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, launch_selftest_math(c->stream, fn, da, db, n, dout));
  HIPP(c, pre, hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_obstacle_distance(clrrt_ctx* c, const double* states, int32_t n, double* out) {
  if (!c || n < 0 || (n > 0 && (!states || !out))) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const char* const pre = "obstacle_distance: ";
  Scratch<double> din, dout;
  HIPP(c, pre, din.alloc(10 * (size_t)n));
  HIPP(c, pre, dout.alloc(n));
  HIPP(c, pre, hipMemcpyAsync(din, states, sizeof(double) * 10 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  const OccGrid og = occ_view(c);
  HIPP(c, pre, launch_obs_distance(c->stream, c->dp, c->obs, din, n, dout, &og));
  HIPP(c, pre, hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_selftest_units(clrrt_ctx* c, int32_t unit, const double* in, int32_t n, double* out) {
  const int K = CLRRT_UNIT_CTRL_K;
  static const int kin[10] = {11, 9, 9, 12, 2, 6, 7, 8, 8, 12 + 6 * K};
  static const int kout[10] = {1, 8, 1, 1 + 3 * CLRRT_UNIT_PROFILE_NMAX, 2, 2, 3, 1, 1 + 3 * CLRRT_UNIT_PROFILE_NMAX,
                               4 + 8 * K};
  if (!c || n < 0 || (n > 0 && (!in || !out)) || unit < 0 || unit > CLRRT_UNIT_CTRL) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const size_t nin = (size_t)kin[unit] * n, nout = (size_t)kout[unit] * n;
  std::vector<BakedObs> baked;
  if (unit == CLRRT_UNIT_OBB) {
    baked.resize(n);
    for (int i = 0; i < n; i++) {
      const double* a = in + 11 * (size_t)i;
      clrrt_obstacle o = {a[4], a[5], a[6], a[7], a[8], a[9], a[10]};
      bake_obstacle(o, baked[i]);
    }
  }
  // per-case parameters: the context's, with the case's goal / vmax / ref_res, derived as
  // clrrt_set_params derives them
  std::vector<DevParams> cps;
  if (unit >= CLRRT_UNIT_FEASIBLE) {
    cps.resize(n);
    for (int i = 0; i < n; i++) {
      const double* a = in + (size_t)kin[unit] * i;
      clrrt_params q = c->params;
      if (unit == CLRRT_UNIT_FEASIBLE) q.ref_res = a[6];
      if (unit == CLRRT_UNIT_GOALBIAS) for (int k = 0; k < 4; k++) q.goal[k] = a[k];
      if (unit == CLRRT_UNIT_GOALREF) { for (int k = 0; k < 4; k++) q.goal[k] = a[k]; q.ref_res = a[7]; }
      if (unit == CLRRT_UNIT_CTRL) { for (int k = 0; k < 4; k++) q.goal[k] = a[5 + k]; q.vmax = a[10]; q.ref_res = a[11]; }
      derive(q, cps[i], c->n_obs);
    }
  }
  const char* const pre = "selftest_units: ";
  Scratch<double> din, dout;
  Scratch<BakedObs> dobs;
  Scratch<DevParams> dcp;
  HIPP(c, pre, din.alloc(nin));
  HIPP(c, pre, dout.alloc(nout));
  if (!baked.empty()) HIPP(c, pre, dobs.alloc(baked.size()));
  if (!cps.empty()) HIPP(c, pre, dcp.alloc(cps.size()));
  HIPP(c, pre, hipMemcpyAsync(din, in, sizeof(double) * nin, hipMemcpyHostToDevice, c->stream));
  if (dobs)
    HIPP(c, pre, hipMemcpyAsync(dobs, baked.data(), sizeof(BakedObs) * baked.size(), hipMemcpyHostToDevice, c->stream));
  if (dcp)
    HIPP(c, pre, hipMemcpyAsync(dcp, cps.data(), sizeof(DevParams) * cps.size(), hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, hipMemsetAsync(dout, 0, sizeof(double) * nout, c->stream));
  HIPP(c, pre, launch_selftest_units(c->stream, unit, din, dobs, n, c->dp, dcp, dout));
  HIPP(c, pre, hipMemcpyAsync(out, dout, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_selftest_collision(clrrt_ctx* c, int32_t path, const double* states, const int32_t* active, int32_t n,
                             double* dist, uint32_t* tests) {
  if (!c || n < 0 || (n > 0 && (!states || !active || !dist || !tests)) || path < CLRRT_COLL_EXHAUSTIVE ||
      path > CLRRT_COLL_COOP)
    return CLRRT_EINVAL;
  RollArgs a = roll_args(c, 0);
  a.ctr = nullptr;
  a.coop_enable = c->roll_coop;
  if (path == CLRRT_COLL_COOP && !roll_coop_applies(a))
    return fail(c, CLRRT_EINVAL, "selftest_collision: a rollout launch would not use the cooperative check here");
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const char* const pre = "selftest_collision: ";
  Scratch<double> din, ddist;
  Scratch<int32_t> dact;
  Scratch<uint32_t> dtests;
  HIPP(c, pre, din.alloc(10 * (size_t)n));
  HIPP(c, pre, ddist.alloc(n));
  HIPP(c, pre, dact.alloc(n));
  HIPP(c, pre, dtests.alloc(n));
  HIPP(c, pre, hipMemcpyAsync(din, states, sizeof(double) * 10 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, hipMemcpyAsync(dact, active, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, launch_selftest_collision(c->stream, a, path, din, dact, n, ddist, dtests));
  HIPP(c, pre, hipMemcpyAsync(dist, ddist, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipMemcpyAsync(tests, dtests, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_debug_grid(clrrt_ctx* c, int32_t info_i[6], float info_f[3], uint32_t* start, uint16_t* items,
                     uint16_t* mov) {
  if (!c || !info_i || !info_f) return CLRRT_EINVAL;
  const ObsGrid& g = c->grid;
  RollArgs a = roll_args(c, 0);
  a.coop_enable = c->roll_coop;
  info_i[0] = g.gw; info_i[1] = g.gh; info_i[2] = g.nitems; info_i[3] = g.nmov;
  info_i[4] = roll_coop_applies(a) ? 1 : 0;
  info_i[5] = c->grid_exempt;
  info_f[0] = g.x0; info_f[1] = g.y0; info_f[2] = g.inv;
  HIPC(c, hipSetDevice(c->device));
  if (start && g.gw > 0)
    HIPC(c, hipMemcpyAsync(start, g.start, sizeof(uint32_t) * ((size_t)g.gw * g.gh + 1), hipMemcpyDeviceToHost, c->stream));
  if (items && g.nitems > 0)
    HIPC(c, hipMemcpyAsync(items, g.items, sizeof(uint16_t) * (size_t)g.nitems, hipMemcpyDeviceToHost, c->stream));
  if (mov && g.nmov > 0)
    HIPC(c, hipMemcpyAsync(mov, g.mov, sizeof(uint16_t) * (size_t)g.nmov, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_nn_batch(clrrt_ctx* c, const clrrt_sample* samples, int32_t n, int32_t mode, int32_t* out_ids,
                   float* out_keys) {
  if (!c || n < 0 || (n > 0 && (!samples || !out_ids))) return CLRRT_EINVAL;
  pf_reset(c);
  ListSet& cur = *c->ls[0];
  if (mode != CLRRT_MODE_EXACT && mode != CLRRT_MODE_BATCH) return CLRRT_EINVAL;
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  memcpy(cur.h_samples, samples, sizeof(clrrt_sample) * n);
  HIPC(c, hipMemcpyAsync(cur.d_samples, cur.h_samples, sizeof(clrrt_sample) * n, hipMemcpyHostToDevice, c->stream));
  int rc = CLRRT_OK;
  if (mode == CLRRT_MODE_EXACT && (rc = ensure_sort_scratch(c, (int64_t)n * c->n_nodes)) != CLRRT_OK) return rc;
  if ((rc = run_nn(c, n, mode == CLRRT_MODE_EXACT ? c->sort_scratch : nullptr)) != CLRRT_OK) return rc;
  HIPC(c, hipMemcpyAsync(out_ids, cur.cand, sizeof(int) * CAND_K * n, hipMemcpyDeviceToHost, c->stream));
  if (out_keys)
    HIPC(c, hipMemcpyAsync(out_keys, cur.ckey, sizeof(float) * CAND_K * n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_round_sizes(clrrt_ctx* c, int64_t* out, int64_t cap, int64_t* n) {
  if (!c || cap < 0 || (cap > 0 && !out)) return CLRRT_EINVAL;
  const int64_t m = (int64_t)c->round_sizes.size();
  for (int64_t i = 0; i < std::min(m, cap); i++) out[i] = c->round_sizes[(size_t)i];
  if (n) *n = m;
  return CLRRT_OK;
}

int clrrt_walk_audit(clrrt_ctx* c, const clrrt_sample* samples, int32_t n, int32_t* out) {
  if (!c || n < 0 || (n > 0 && (!samples || !out))) return CLRRT_EINVAL;
  pf_reset(c);
  ListSet& cur = *c->ls[0];
  if (n > c->cap.max_batch) return fail(c, CLRRT_ECAPACITY, "batch larger than max_batch");
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const NnSetup su = nn_setup(c);
  if (!walk_serves(c, su)) return fail(c, CLRRT_ESTATE, "the walk does not serve this tree (too small or no region)");
  int rc = ensure_walk(c);
  if (rc != CLRRT_OK) return rc;
  memcpy(cur.h_samples, samples, sizeof(clrrt_sample) * n);
  HIPC(c, hipMemcpyAsync(cur.d_samples, cur.h_samples, sizeof(clrrt_sample) * n, hipMemcpyHostToDevice, c->stream));
  c->nnw_built.n = -1;
  HIPC(c, launch_nn_walk_build(c->stream, c->nn, (int)c->n_nodes, su.fr, su.x0, su.y0, su.x1, su.y1, c->nnw));
  const char* const pre = "clrrt_walk_audit: ";
  Scratch<int> d_out;
  HIPC(c, d_out.alloc(20 * (size_t)n));  // (HIPC, not HIPP: this failure never carried the prefix)
  HIPP(c, pre, launch_walk_audit(c->stream, cur.d_samples, n, c->nn, (int)c->n_nodes, c->dp, su.fr, c->nnw, d_out));
  HIPP(c, pre, hipMemcpyAsync(out, d_out, sizeof(int32_t) * 20 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

int clrrt_debug_walk_index(clrrt_ctx* c, int64_t first, int64_t count, int32_t fused, double hdr[9], float* P,
                           float* Q, float* CE, int32_t* ID, int32_t* HEAD, int32_t* trun, void* tiles, void* supers,
                           int32_t* roster) {
  if (!c || !hdr) return CLRRT_EINVAL;
  if (first < 0 || count <= 0 || first > c->n_nodes || count > c->n_nodes - first)
    return fail(c, CLRRT_EINVAL, "debug_walk_index: node range outside the tree");
  pf_reset(c);
  HIPC(c, hipSetDevice(c->device));
  const NnSetup su = nn_setup(c);
  const bool whole = !fused && first == 0 && count == c->n_nodes;
  if (!su.region_ok || c->n_nodes < c->nnw_min_nodes || (!fused && !whole && count < c->nnw_min_nodes))
    return fail(c, CLRRT_ESTATE, "the walk does not serve this tree (too small or no region)");
  int rc = CLRRT_OK;
  WalkBufs* w = nullptr;
  if (fused) {
    if ((rc = alloc_walk_delta(c)) != CLRRT_OK) return rc;
    w = &c->nnw_d;
    if (count > w->cap_nodes) return fail(c, CLRRT_ECAPACITY, "debug_walk_index: range beyond the appended-node set");
    HIPC(c, launch_nn_delta_index(c->stream, c->nn, (int)first, (int)count, su.fr, su.x0, su.y0, su.x1, su.y1, *w));
  } else if (whole) {
    if ((rc = ensure_walk(c)) != CLRRT_OK) return rc;
    w = &c->nnw;
    c->nnw_built.n = -1;
    HIPC(c, launch_nn_walk_build(c->stream, c->nn, (int)count, su.fr, su.x0, su.y0, su.x1, su.y1, *w));
  } else {
    w = &c->nnw_r;
    if ((rc = ensure_walk_set(c, *w)) != CLRRT_OK) return rc;
    c->nnr_built.n = -1;
    HIPC(c, launch_nn_walk_build(c->stream, c->nn, (int)count, su.fr, su.x0, su.y0, su.x1, su.y1, *w, nullptr,
                                 (int)first));
  }
  const char* const pre = "debug_walk_index: ";
  const size_t nt = (size_t)walk_tile_count(count), ns = (size_t)walk_super_count(count), np = nt * 32;
  NnRec r0;
  HIPP(c, pre, hipMemcpyAsync(&r0, c->nn, sizeof(NnRec), hipMemcpyDeviceToHost, c->stream));
  if (P) HIPP(c, pre, hipMemcpyAsync(P, w->P, sizeof(float4) * np, hipMemcpyDeviceToHost, c->stream));
  if (Q) HIPP(c, pre, hipMemcpyAsync(Q, w->Q, sizeof(float4) * np, hipMemcpyDeviceToHost, c->stream));
  if (CE) HIPP(c, pre, hipMemcpyAsync(CE, w->CE, sizeof(float) * np, hipMemcpyDeviceToHost, c->stream));
  if (ID) HIPP(c, pre, hipMemcpyAsync(ID, w->ID, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
  if (HEAD) HIPP(c, pre, hipMemcpyAsync(HEAD, w->HEAD, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
  if (trun) HIPP(c, pre, hipMemcpyAsync(trun, w->trun, sizeof(int2) * nt, hipMemcpyDeviceToHost, c->stream));
  if (tiles) HIPP(c, pre, hipMemcpyAsync(tiles, w->tiles, sizeof(WalkTile) * nt, hipMemcpyDeviceToHost, c->stream));
  if (supers) HIPP(c, pre, hipMemcpyAsync(supers, w->supers, sizeof(WalkTile) * ns, hipMemcpyDeviceToHost, c->stream));
  if (roster) {
    memset(roster, 0, sizeof(int32_t) * 66);
    roster[1] = -1;
    if (!fused && w->roster)
      HIPP(c, pre, hipMemcpyAsync(roster, w->roster, sizeof(int32_t) * 66, hipMemcpyDeviceToHost, c->stream));
  }
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  hdr[0] = (double)np; hdr[1] = (double)nt; hdr[2] = (double)ns;
  hdr[3] = su.fr.ox; hdr[4] = su.fr.oy; hdr[5] = (double)su.fr.delta;
  hdr[6] = (double)su.fr.delta;  // the builders' slack is the frame's delta
  hdr[7] = (double)(float)(r0.x - su.fr.ox); hdr[8] = (double)(float)(r0.y - su.fr.oy);  // k_walk_tiles' R
  return CLRRT_OK;
}

int clrrt_selftest_walk(clrrt_ctx* c, int32_t fn, const float* in, int32_t n, float* out) {
  static const int kin[5] = {3, 3, 21, 2, 2};
  static const int kout[5] = {2, 2, 2, 2, 3};
  if (!c || n < 0 || (n > 0 && (!in || !out)) || fn < 0 || fn > 4) return CLRRT_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (n == 0) return CLRRT_OK;
  const size_t nin = (size_t)kin[fn] * n, nout = (size_t)kout[fn] * n;
  const char* const pre = "selftest_walk: ";
  Scratch<float> din, dout;
  HIPP(c, pre, din.alloc(nin));
  HIPP(c, pre, dout.alloc(nout));
  HIPP(c, pre, hipMemcpyAsync(din, in, sizeof(float) * nin, hipMemcpyHostToDevice, c->stream));
  HIPP(c, pre, hipMemsetAsync(dout, 0, sizeof(float) * nout, c->stream));
  HIPP(c, pre, launch_selftest_walk(c->stream, fn, din, n, dout));
  HIPP(c, pre, hipMemcpyAsync(out, dout, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
  HIPP(c, pre, hipStreamSynchronize(c->stream));
  return CLRRT_OK;
}

}  // extern "C"
