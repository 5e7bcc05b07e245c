// Host-side objects behind the opaque C handles.
#pragma once
#include "common.h"
#include "kernels.h"
#include "dispatch.h"
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

namespace mse {

// growable device buffer (grows by hipMalloc + free; contents are NOT preserved)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
    ~DevBuf() { release(); }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// the thread's current device for the length of a call that must build on another one (filter_api.hip, group_api.hip)
struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// growable pinned host staging: grows to max(2 x bytes, floor) by hipHostMalloc + free (contents are NOT preserved).  Move-only: it
// lives in objects that are moved (a vector of worker contexts), never copied
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    int ensure(size_t bytes, size_t floor);
    void release();
    ~PinBuf() { release(); }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// device scratch of one run of build_graph_on_device (graph_build.hip): visited sets and lists, staged lists, error words, the
// back-edge grouping.  mse_build_graph makes one per call; mse_graph_insert_rows keeps one on the searcher
struct BuildScratch {
    DevBuf cnts, bm, vli, vls, stg, stg_len, err, grp;
};

int device_cu_count();

// one level of the selection tournament (topk.hip)
struct LevelRef {
    KeyKind kind;
    const void* ptr;
    size_t q_stride, e_stride, n;  // element (q, i) lives at ptr[q*q_stride + i*e_stride]
    bool group_major;              // float [n][nq_pad] as written by the MFMA scan
    int nq_pad;
};

}  // namespace mse

struct mse_searcher;
struct mse_build_config;
struct mse_graph;
namespace mse {
// Tournament descent: ids of the k best level-0 entries per query in *sel_out ([nq][k], best first);
// their raw keys in keys_out when it is not null.  Uses the searcher's scratch and stream.
int descend(mse_searcher* s, const LevelRef& l0, int nq, int k, uint32_t** sel_out, void* keys_out);
// workspace-only searcher (no base vectors): scratch + stream for the PQ scan
mse_searcher* scratch_searcher_new();
}  // namespace mse

struct mse_base {
    const uint16_t* dev = nullptr;
    size_t n = 0, d = 0;
    bool owned = false;
    int n_cu = 256;
    int device = 0;            // HIP ordinal the rows live on (the thread's current device when the base was made)
    // the coalescer that MSE_MODE_AUTO host-pointer searches of every thread meet in (dispatch.hip), made on first use
    mutable std::mutex disp_mu;
    mutable struct mse_dispatcher* disp = nullptr;
    mutable bool disp_failed = false;   // it could not be made once: AUTO calls are answered directly from then on
    // max row norm (float bits) for the MFMA certificate, computed on first use
    mutable std::mutex norm_mu;
    mutable uint32_t* norm_bits_dev = nullptr;
    mutable bool norm_ready = false;
};

// row filter of the filtered brute-force search (filter.hip; immutable once made)
struct mse_filter {
    int device = 0;              // HIP ordinal the bitmap lives on
    size_t n_rows = 0;           // rows it speaks for; rows at or past it are excluded
    size_t n_words = 0;          // bitmap words: one per 32-row group, padded to whole 256-row scan tiles
    size_t count = 0;            // allowed rows
    uint32_t* words = nullptr;   // device bitmap
    uint32_t* ids = nullptr;     // device: the allowed rows, ascending (count of them)
};

// row grouping of the grouped search (group.hip, group_api.hip; immutable once made)
struct mse_groups {
    int device = 0;                // HIP ordinal the array lives on
    size_t n_rows = 0;             // rows it speaks for; rows at or past it are groups of their own
    size_t count = 0;              // distinct ids + MSE_GROUP_NONE rows
    uint32_t* group_of = nullptr;  // device [n_rows]: group id (< n_rows) or MSE_GROUP_NONE
};

namespace mse {
// one query's outputs of the fused request path (any of the counter pointers may be null)
struct QueryDst {
    uint32_t* ids; int64_t* scores; uint32_t *n_visited, *cmps, *pq_cmps; size_t k;
};
}  // namespace mse

namespace mse {
// the self-join's state on a searcher (join_api.hip): what mse_join_stats reads -- shared with the pair lists the searcher made, so that a
// list's keep-first resolution can report its rounds after the call that made it -- the test hook's buffer size and the call scratch
struct JoinStats { std::atomic<uint64_t> v[6]; JoinStats() { for (auto& x : v) x.store(0); } };
struct JoinState {
    std::shared_ptr<JoinStats> stats = std::make_shared<JoinStats>();
    uint64_t cand_cap = 0;       // nominated pairs one launch may store; 0 = default
    DevBuf cand, tiles, tile_base, counters, row_count;
    // optional measurement (mse_join_timing, for scripts/near_duplicate_probe.py): HIP-event milliseconds of the last call's tile
    // launches, re-score launches and list build; while it is on the call waits once more per launch
    bool timing = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0};
};
}  // namespace mse

// result of mse_join_self / mse_join_cross (join.hip, join_api.hip; the list is immutable, a self list's keep-first resolution is made on
// first use and kept).  A cross list (kind 1) is a CSR over the INCOMING rows (n_rows of them); its lo ids are rows of the resident base
struct mse_pairs {
    int device = 0;
    int kind = 0;                            // 0: self list, 1: cross list
    size_t base_rows = 0;                    // rows of the resident base (a self list: n_rows)
    size_t n_rows = 0, count = 0;
    unsigned long long* offsets = nullptr;   // device [n_rows + 1]: the CSR over hi
    uint32_t *lo = nullptr, *hi = nullptr;   // device [count], canonical order
    int64_t* scores = nullptr;               // device [count]
    std::shared_ptr<mse::JoinStats> stats;
    std::mutex mu;                           // guards the resolution below
    bool resolved = false;
    uint64_t rounds = 0;
    uint32_t *rep = nullptr, *labels = nullptr, *dup_words = nullptr;   // device [n_rows] | [n_rows] | whole 256-row tiles of bitmap
};

struct mse_searcher {
    const mse_base* base = nullptr;
    mse::JoinState join;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int n_cu = 256;
    mse::DevBuf q_stage;      // padded queries for one pass
    mse::DevBuf scores;       // [pass_q][n] i64 / f32 level 0 (exact mode)
    mse::DevBuf levels[6];    // tournament levels above level 0
    mse::DevBuf sel_a, sel_b; // selected ids ping-pong
    mse::DevBuf sel_keys;     // keys of the final selection
    mse::DevBuf out_scores, out_ids;  // device outputs for the host-pointer API
    mse::DevBuf gmax;         // MFMA group maxima [n_groups][nq_pad]
    mse::DevBuf cand_ids, cand_scores, gkeys, eps, margin;
    mse::DevBuf misc, qpacked;
    mse::DevBuf pq4;          // four-query PQ scan: the packed 12-bit table (136 KiB) + the four queries' certificate parameters
    mse::DevBuf wq, wg, widx, wout;   // per-query widening of the MFMA pass: the compact set's queries, group maxima, indices, results
    mse::PinBuf margin_pin;   // certificate margins of an MFMA round on their way to the host
    mse::DevBuf thr;          // [2][nq] u64: k-th best score key of each tournament level, the floor of the level below
    // after descend(): per query a LOWER BOUND of the k-th best level-0 key (sortable u64, 32-bit keys in the top half), or null.
    // It is the radix select's threshold prefix: the k-th key itself when the search ran through every score digit, the k-th key
    // with its low digits zeroed when a bucket was taken whole, 0 when no more than k entries exist.  At least k entries reach it,
    // which is all a floor needs (api_pq.hip); tests/test_gpu_topk_select.py pins `<= k-th key`, not equality.
    const unsigned long long* last_kth = nullptr;
    mse::DevBuf pool[16];     // scratch of the batched graph searches (kept between calls: no hipMalloc on the query path)
    // a filter per query (beam_search.hip, mse_disk_query_topk_filtered_each): the launch's table [nq] of (bitmap, rows), and the host
    // staging of a call that splits into classes -- gathered inputs, the classes' filter pointers and output destinations
    mse::DevBuf flt_tab;
    std::vector<unsigned char> flt_host;   // the table on its way to the device: lives as long as the copy may be in flight
    mse::PinBuf each_stage;
    std::vector<const mse_filter*> each_filters;
    std::vector<mse::QueryDst> each_dsts;
    mse::DevBuf del_scratch[10];   // scratch of mse_graph_delete_rows (graph_delete.hip), kept between calls for the same reason
    mse::DevBuf ins_scratch[8];    // scratch of mse_graph_insert_rows (graph_insert.hip): slots, staging slabs, codes, flags
    mse::BuildScratch ins_build;   // ... and of its link step
    uint32_t last_widened = 0, last_max_groups = 0;
    // grouped search (bruteforce.hip grouped_topk_dev, api_pq.hip): the candidate prefix [nq][k'] (ids | keys), the collapse's positions
    // and counts, the compact set of the queries that go on, the dense path's group table (best keys | best ids)
    mse::DevBuf grp_ids, grp_keys, grp_pos, grp_reps, grp_q, grp_q2, grp_idx, grp_best;
    mse::PinBuf grp_pin;      // representative counts and list tails on their way to the host
    uint32_t last_grouped[3] = {0, 0, 0};   // of the last grouped call: queries answered from the first prefix, a widened one, the dense path
    // optional measurement of the grouped search (mse_searcher_grouped_timing, for scripts/grouped_search_probe.py): HIP-event
    // milliseconds of [0] the collapse kernel of the prefix rounds, and of the dense passes [1] the score pass, [2] the group atomics and
    // the demotion, [3] the selection with its collapse and gather
    bool grp_timing = false;
    hipEvent_t grp_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double grp_ms[4] = {0.0, 0.0, 0.0, 0.0};
    // thresholded group maxima of the 320-query pass (bruteforce.hip mfma_pass; mse_searcher_set_sparse_maxima): mode 0 auto, 1 off, 2 forced;
    // every sparse_stride-th 256-row tile is the sample (stride - 1 a power of two); sparse_cap survivors per query at most
    int sparse_mode = 0;
    uint32_t sparse_stride = 33, sparse_cap = 8192;
    uint32_t last_sparse_passes = 0, last_sparse_fallbacks = 0, last_sparse_max_list = 0;   // of the last MFMA-mode call, as last_widened
    mse::DevBuf sp_dense;     // the sample's dense maxima [sample groups][320]
    mse::DevBuf sp_lists;     // thresholds [320] f32 | survivor counts [320] u32 | group ids [320][cap] u32 | maxima [320][cap] f32
    mse::DevBuf sp_wlists;    // the same for the widening's compact set
    mse::PinBuf sp_pin;       // the survivor counts on their way to the host
    // optional HIP-event timing of the dominant (scan) kernel, for bench.py's roofline line
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double scan_ms_total = 0.0;
    uint64_t scan_launches = 0;
    // optional measurement of the graph search kernel (mse_searcher_beam_timing, for bench.py's gather roofline): HIP events around
    // beam_search_kernel and device totals of what it gathered -- [0] rows scored exactly (2304-byte row gathers: fetched nodes and
    // exactly scored neighbours), [1] fetched nodes (adjacency lists read), [2] neighbours scored by ADC (64-byte code gathers)
    bool beam_timing = false;
    hipEvent_t bev0 = nullptr, bev1 = nullptr;
    double beam_ms_total = 0.0;
    uint64_t beam_launches = 0, beam_queries = 0;
    mse::DevBuf beam_tot;
    // optional measurement of mse_graph_compact's row-gather kernel (mse_searcher_compact_timing): HIP events around that launch, the
    // last call's milliseconds
    bool compact_timing = false;
    double compact_gather_ms = 0.0;
    // event pairs of the PQ scan launches of one batch call (several per call on this searcher's stream), read when the call ends
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // pinned host staging of the fused request path (ONE download per call: scores, ids and counters) and the event of
    // mse_searcher_wait_stream
    mse::PinBuf pin;
    hipEvent_t ev_wait = nullptr;
};

struct mse_pq {
    size_t n_centroids = 0, d = 0, dpc = 0, n_chunks = 0;
    float* centroids = nullptr;  // device [n_centroids][d]
    float* transform = nullptr;  // device [d][d]
    float* transform_t = nullptr;  // device [d][d], transposed copy for the one-vector (query) path
    std::mutex mu;
    mse::DevBuf a, b, c;              // call scratch (guarded by mu)
    mse_searcher* scratch = nullptr;  // stream + scratch for scan calls that bring no searcher (guarded by mu; made on first use)
    mse_searcher* lane2 = nullptr;    // second and third stream of the batched scan; bound to the base of the call that made them
    mse_searcher* lane3 = nullptr;
    mse::DevBuf t2, lut2, qf2, qf3;   // their transformed query, table and f16 queries
    bool avoid8 = false;              // eight-per-pass (8-bit tables) gave too many uncertified queries on this data: stay with four per pass
    uint32_t last_uncertified = 0;    // four-query scan: queries of the last batch whose certificate failed (re-run through the exact scan)
    int device = 0;                   // HIP ordinal the quantiser was loaded on
    std::mutex co_mu;                 // guards the creation of `co`
    mse::Coalescer* co = nullptr;     // meeting point of one-query mse_pq_scan_topk calls from many threads (api_pq.hip), made on first use
    bool timing = false;              // HIP-event timing of the four-query scan kernel (mse_pq_scan_timing), for bench.py's roofline
    double scan_ms_total = 0.0;
    uint64_t scan_launches = 0;
    double span_ms_total = 0.0;       // first scan start .. last scan end of the batch calls with >= 4 scans (mse_pq_scan_sustained)
    uint64_t span_scans = 0;
    mse::PinBuf pin;                  // pinned host staging of the scan entry points (one upload + one download per call, both
                                      // truly asynchronous: a pageable source makes the runtime stage and block per copy)
};

struct mse_codes {
    uint8_t* codes = nullptr;    // device [n][code_size]
    uint8_t* desc = nullptr;     // device [n][n_desc] or null
    size_t n = 0, code_size = 0, n_desc = 0;
};

namespace mse {
// a filter may be used on base b: same device, no longer than the rows (filter_api.hip); 0, or -1 with the error set
int check_filter(const mse_base* b, const mse_filter* f);
// the sparse side of the crossover: nq queries through the filter's id list cost less than the masked scan over all rows (bruteforce.hip)
bool filter_sparse(const mse_base* b, const mse_filter* f, size_t nq);
// what MSE_MODE_AUTO resolves to for nq queries (f: the call's filter or null; coalesced: the call is a pass of the base's coalescer) --
// the one statement of the rule (bruteforce.hip)
int bruteforce_auto_mode(const mse_base* b, const mse_filter* f, size_t nq, bool coalesced);
// the body of mse_bruteforce_topk_f16_dev (f = null) and mse_bruteforce_topk_filtered_f16_dev, validation included (bruteforce.hip)
int bruteforce_topk_dev(mse_searcher* s, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode, uint64_t id_offset,
                        void* scores_dev, void* ids_dev);
// the body of mse_bruteforce_topk_grouped_f16_dev (g non-null, f may be null), validation included (bruteforce.hip)
int grouped_topk_dev(mse_searcher* s, const mse_groups* g, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode,
                     uint64_t id_offset, void* scores_dev, void* ids_dev);
// One exact pass of <= 8 queries (staged, padded, in s->q_stage) over the rows ids[0 .. n) -- ascending; null: rows 0 .. n -- and the
// exact top-k of each: i64 scores in the reference order, (score desc, id asc), padding INT64_MIN / ID_NONE; a row that is not listed is
// absent.  bias (optional, needs ids): the descriptor product of every listed row is added to its score before the selection.
// g (optional; then nq_pass <= dense_pass_queries(g->n_rows, 12)): one result per group of g, the grouped search's dense pass over these
// rows and scores, into row dst_rows[j] (device; null: j) of the outputs.
struct ListBias { const uint8_t* desc; int n_desc; const float* scales_dev; };   // scales_dev: [nq_pass][n_desc] on the device
int exact_pass_list(mse_searcher* s, int nq_pass, int k, uint64_t id_offset, int64_t* out_scores, uint32_t* out_ids, size_t out_stride,
                    const uint32_t* ids, size_t n, const ListBias* bias, const mse_groups* g = nullptr, const uint32_t* dst_rows = nullptr);
// a grouping may be used on base b: same device, no longer than the rows (group_api.hip); 0, or -1 with the error set
int check_groups(const mse_base* b, const mse_groups* g);
// The arguments of a PQ flat scan (api_pq.hip), in the order every entry point reports them: the handles; of a filtered call (fa) the
// filter -- given, no longer than the codes, on the quantiser's device -- and its mode; code size against the quantiser; max(r, k)
// within the tournament's limit; of a searcher with a base, its length against the codes and its width against the quantiser.
// An unfiltered call with nothing to do (nq or k zero) is asked for no more than handles and code size.  0, or -1 with the error set.
struct PqFilterArg { const mse_filter* f; int mode; };
int check_pq_scan(const mse_pq* pq, const mse_codes* c, const mse_searcher* s, size_t nq, size_t r, size_t k, const PqFilterArg* fa);
// ... and the two of its checks that stand alone: a sharded call has no single quantiser to hand and checks its numbers before its
// shards check the rest
int check_pq_mode(int mode);
int check_pq_r(size_t r, size_t k);
// The exact re-score of a PQ scan's top-r (query_disk_index.rs:168-170,477): out[i] = f16 query . base row ids[i], per_query ids to a
// query of q16, + the descriptor bias only when scales AND descriptors are there (api_pq.hip)
int exact_rescore(const mse_base* b, const mse_codes* c, const float* scales_dev, const void* q16, const uint32_t* ids, size_t n, size_t per_query,
                  int64_t* out, hipStream_t st);
// the dense path's scratch is bounded: queries one dense pass may take (1 .. 8) with a group table of g_len entries of `bytes` bytes each
int dense_pass_queries(size_t g_len, size_t bytes);
// the collapse half of a round of the grouped search's prefix path (bruteforce.hip), shared with the flat index
int grouped_collapse_round(mse_searcher* s, const mse_groups* g, int key_bytes, size_t nq, size_t kp, int k, uint64_t id_offset,
                           const std::vector<uint32_t>* dst, void* out_keys, uint32_t* out_ids, size_t out_stride, std::vector<uint32_t>* open_out,
                           std::vector<uint32_t>* open_reps);
// the rounds of the prefix path over the nq queries at q (rows of row_bytes), shared by the brute force and the flat index (bruteforce.hip):
// round(queries, count, k', output rows or null, &open, &open_reps) runs one search + grouped_collapse_round; dense(queries, count,
// output rows) answers what the rounds left.  Counts the queries per path into s->last_grouped
using GroupedRound = std::function<int(const void*, size_t, size_t, const std::vector<uint32_t>*, std::vector<uint32_t>*, std::vector<uint32_t>*)>;
using GroupedDense = std::function<int(const void*, size_t, const std::vector<uint32_t>&)>;
int grouped_prefix_drive(mse_searcher* s, const void* q, size_t row_bytes, size_t nq, size_t k, const GroupedRound& round, const GroupedDense& dense);
// largest row norm of the base (x 1.0001), computed once and kept on the device as float bits (b->norm_bits_dev)
int ensure_base_norm(const mse_base* b, hipStream_t st);
// Bound, in the fixed-point scale, on |MFMA f16 sum - fast_dot| for two rows of b (graph_build.hip; the certificate of DESIGN.md 3.2):
// *eps_fix = 0 when none can be stated (a width that is no multiple of 64, a non-finite row)
int mfma_pair_bound(const mse_base* b, hipStream_t st, long long* eps_fix);
// the same for a pair with one row from each of two bases of one width: the one-base formula over the element-wise maximum of their
// three norm figures
int mfma_cross_bound(const mse_base* a, const mse_base* b, hipStream_t st, long long* eps_fix);
// error bound of the matrix-core products robust_prune may decide by (graph_build.hip): *eps_fix = 0 means exact dots only
int prune_mfma_eps(const mse_base* b, const ::mse_build_config* cfg, hipStream_t st, long long* eps_fix);
// the limits mse_build_graph sets on the searcher, the graph and the config (graph_build.hip); 0, or -1 with the error set
int check_build_config(const mse_searcher* s, const ::mse_graph* g, const ::mse_build_config* cfg, const char* who);
// mse_build_graph after its validation, over an order that is already on the device: order_dev[0 .. n_order) in batches of `batch`
// (>= 1) from `medioid`, scratch in sc, errors prefixed with `who`; *n_batches (may be null) = batches run.  The caller has checked
// the config, the order and the graph's edges.  Returns with the searcher's stream drained
int build_graph_on_device(mse_searcher* s, ::mse_graph* g, const uint32_t* order_dev, size_t n_order, size_t batch, uint32_t medioid,
                          const ::mse_build_config* cfg, BuildScratch& sc, const char* who, size_t* n_batches);
// device memory the batched graph searches may spend on visited sets per launch: half of the free HBM, 256 MiB .. 64 GiB
// (MSE_VISITED_BUDGET_KB overrides, for tests)
size_t visited_budget_bytes();
}  // namespace mse

struct mse_graph {
    uint32_t* adj = nullptr;   // device [n][max_deg]
    uint32_t* deg = nullptr;   // device [n]
    uint8_t* has_url = nullptr;  // device [n] or null (= all)
    size_t n = 0, max_deg = 0;
    // rows removed by mse_graph_delete_rows (graph_delete.hip): one bit per node on the device (null until the first delete) and how many
    uint32_t* deleted = nullptr;
    size_t n_deleted = 0;
    // meeting point of the ONE-query calls of mse_disk_search_batch(_f32) from many threads (beam_search.hip), made on first use
    // and of the small calls of mse_disk_query_topk(_f32) (round 5): the whole request path of every waiting caller in one
    // submission, on a searcher and pinned staging that belong to the WORKER (one set per worker thread)
    mutable std::mutex co_mu;
    mutable mse::Coalescer* co = nullptr;
    mutable std::atomic<mse::Coalescer*> co_fast{nullptr};   // == co once made: the request threads' lock-free way to it
    struct WorkerCtx {
        mse_searcher* s = nullptr;   // made on first use over the callers' base
        mse::PinBuf pin;             // gathered inputs (queries, scales, starts, tables)
        std::vector<mse::QueryDst> dsts;   // where each gathered query's results go
        std::vector<const mse_filter*> filters;   // each gathered query's filter, when the sharers' filters differ
    };
    mutable std::vector<WorkerCtx> co_ctx;
    // what the sharing rule decides (mse_graph_coalescer_groups): groups of requests that ran as ONE submission each -- a gathered
    // batch is split into them by shares_with -- and the requests in them
    mutable std::atomic<uint64_t> co_groups{0}, co_group_requests{0};
    size_t co_max_queries = 0;       // mse_graph_set_coalescer: 0 = defaults (1024 queries per pass, 200 us, two workers)
    uint32_t co_max_wait_us = 0;
    int co_workers = 0;
    // entry table of the fused request path (beam_search.hip), one of two kinds:
    //   mse_graph_set_entries          copies of the entry records' vectors + their node ids; entry = exact top-1 over the copies
    //   mse_graph_set_entry_centroids  the reference's rule: f32 shard centroids as keys (transposed [d][n_entries]) + medioid ids
    // Request-path calls hold entry_lock shared for their duration; replacing the table takes it exclusively, and so does
    // mse_graph_delete_rows / _restore_rows while it rewrites lists and flags.
    uint16_t* entry_rows = nullptr;
    uint32_t* entry_ids = nullptr;
    size_t n_entries = 0;
    mse_base* entry_base = nullptr;
    float* entry_keys_t = nullptr;
    size_t entry_keys_d = 0;
    mutable mse::SharedExclusive entry_lock;
    // runtime de-duplication of the request path (src/query_disk_index.rs:482-527) inside mse_disk_query_topk(_f32): 0 = off
    float dedup_threshold = 0.0f;
    // searchers over the entry rows: a fused call borrows one for its duration (its scratch is in use until the call's stream is
    // drained), so that calls from several threads -- each with its own searcher and stream -- overlap instead of queueing
    mutable std::vector<mse_searcher*> entry_pool;
    mutable std::mutex entry_mu;
};
