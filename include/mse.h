/*
 * mse.h -- C ABI of libmse_hip.so: the MI355X (gfx950) scoring hot path of meme-search-engine.
 *
 * Drop-in boundary.  Every entry point names the reference interface it replaces (paths are
 * relative to the reference checkout).  A Rust maintainer binds these with an `extern "C"`
 * block (INTEGRATION.md shows the stubs); nothing here mentions torch, HIP or C++ types.
 *
 * Conventions
 *   - All functions returning `int` return 0 on success, non-zero on failure; the message is
 *     available from mse_last_error() (thread-local).  Nothing aborts or throws across the ABI.
 *   - f16 data is passed as uint16_t IEEE binary16 bit patterns (Rust `half::f16` is
 *     repr(transparent) over u16).
 *   - Scores are i64 fixed point, `(f32 * 2^32) as i64`, exactly as diskann::vector produces
 *     (diskann/src/vector.rs:46-47,408-416).
 *   - Pointers named *_dev are device (HBM) pointers; all others are host pointers.  The caller
 *     owns every buffer it passes in; the library keeps no caller pointer after a call returns
 *     except for the *_wrap_device constructors, which borrow.
 *   - Handles are thread-compatible: an mse_base / mse_codes / mse_pq / mse_index may be shared
 *     read-only by any number of threads; each searching thread owns its own mse_searcher
 *     (mirrors the reference: one `Scratch` + `Rc<Index>` per thread over shared `Arc` maps,
 *     src/query_disk_index.rs:714-731).
 *   - Tie order: equal scores are ordered by ascending id (the reference leaves it unspecified:
 *     sort_unstable_by_key, src/query_disk_index.rs:271).
 */
#ifndef MSE_H
#define MSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define MSE_ID_NONE 0xFFFFFFFFu

/* ---- runtime ------------------------------------------------------------------------- */
const char* mse_last_error(void);
int mse_device_count(void);
int mse_set_device(int ordinal);                 /* selects the HIP device for this thread */
int mse_device_synchronize(void);
int mse_device_mem_info(size_t* free_bytes, size_t* total_bytes);
const char* mse_version(void);

/* ---- fixed-point scale: diskann/src/vector.rs:408-416 ---------------------------------- */
int64_t mse_scale_dot_f32(float x);              /* scale_dot_result */
int64_t mse_scale_dot_f64(double x);             /* scale_dot_result_f64 */

/* ---- base vectors: diskann::vector::VectorList (vector.rs:118-186) kept resident in HBM - */
typedef struct mse_base mse_base;
mse_base* mse_base_from_host(const uint16_t* data, size_t n_rows, size_t d);      /* copies */
mse_base* mse_base_wrap_device(const void* data_dev, size_t n_rows, size_t d);    /* borrows; see mse_base_rows_changed */
mse_base* mse_base_generate(uint32_t seed, uint64_t first_row, size_t n_rows, size_t d); /* synthetic rows made on the device */
void mse_base_free(mse_base* b);
size_t mse_base_len(const mse_base* b);
size_t mse_base_dim(const mse_base* b);
const void* mse_base_device_ptr(const mse_base* b);
int mse_base_read_rows(const mse_base* b, size_t first_row, size_t n_rows, uint16_t* out); /* D2H, for spot checks */
/* A base caches its largest row norm (the bound behind the MFMA scan's exactness certificate and the
 * graph build's).  Borrowed memory must stay unchanged while searches run; after rewriting rows of a
 * wrapped base call this (with no search in flight) so the bound is measured again on next use. */
int mse_base_rows_changed(mse_base* b);

/* fast_dot_noprefetch(x, y) / fast_dot(x, y, _) -- diskann/src/vector.rs:255-306,192-252.
 * Host slices in, one i64 out, computed on the device in the reference's summation order. */
/* NB: one call = two uploads, one launch, one download (tens of microseconds): it pins the arithmetic of
 * the interface for parity tests and documents it; production scoring goes through mse_score_rows_f16 /
 * the searches, which keep rows resident and batch the work. */
int mse_fast_dot_f16(const uint16_t* x, const uint16_t* y, size_t n, int64_t* out);

/* ---- searcher: per-thread scratch + stream (reference: `Scratch`, lib.rs:157-175 and
 * query_disk_index.rs:116-123) --------------------------------------------------------- */
typedef struct mse_searcher mse_searcher;
mse_searcher* mse_searcher_new(const mse_base* b);
void mse_searcher_free(mse_searcher* s);
/* HIP stream the searcher launches on (void* = hipStream_t); default: its own stream. */
int mse_searcher_set_stream(mse_searcher* s, void* hip_stream);
void* mse_searcher_stream(const mse_searcher* s);

#define MSE_MODE_AUTO 0   /* host-pointer searches of at most one pass (mse_queries_per_pass_max): coalesced across threads on a
                             worker the base owns (mse_dispatcher below; the caller's stream, scan timing and last_stats are not
                             involved -- mse_dispatcher_searcher has the worker's).  Larger host-pointer batches, device-pointer
                             searches, and every search if that worker could not be made: on the caller's searcher, exact scan
                             for <= 8 queries, batched MFMA scan above that */
#define MSE_MODE_EXACT 1  /* every row scored in the reference order on the vector ALU */
#define MSE_MODE_MFMA 2   /* f16 MFMA scan for candidates + exact re-score + certificate */

/* Most queries one matrix-core pass over the rows serves at vector width d (320; 256 when d / 64 is odd): batches are cut into
 * passes of this size, and it is the dispatcher's default gather size.  Callers that size their own batches gain nothing
 * from going beyond a multiple of it. */
size_t mse_queries_per_pass_max(size_t d);

/* Brute-force top-k: the scan + ranking of `evaluate` (src/query_disk_index.rs:262-273) for a
 * batch of f16 queries.  scores/ids are [nq][k], best first; unfilled slots (k > n_rows) hold
 * INT64_MIN / MSE_ID_NONE.  Returned ids/scores are identical in every mode. */
int mse_bruteforce_topk_f16(mse_searcher* s, const uint16_t* queries, size_t nq, size_t k, int mode,
                            int64_t* scores, uint32_t* ids);
/* Same with device-resident queries/outputs, asynchronous on the searcher's stream.
 * id_offset is added to every returned id (global id = local id + shard offset). */
int mse_bruteforce_topk_f16_dev(mse_searcher* s, const void* queries_dev, size_t nq, size_t k, int mode,
                                uint64_t id_offset, void* scores_dev, void* ids_dev);
/* All n_rows exact scores of one query (what `matches` holds before the sort, :263-269). */
int mse_bruteforce_scores_f16(mse_searcher* s, const uint16_t* query, int64_t* scores);
/* rank[i] = position of row ids[i] in the (score desc, id asc) order of one query; the
 * rank lookup of evaluate (:271-273,309-316). */
int mse_bruteforce_ranks_f16(mse_searcher* s, const uint16_t* query, const uint32_t* ids, size_t n_ids,
                             uint32_t* ranks);
/* Gather-and-score: out[i] = fast_dot(query, base[ids[i]]) -- the neighbour loop of the in-RAM
 * search (diskann/src/lib.rs:201-207) and the fetched-node re-score (query_disk_index.rs:168-169).
 * ids >= n_rows give INT64_MIN. */
int mse_score_rows_f16(mse_searcher* s, const uint32_t* ids, size_t n_ids, const uint16_t* query, int64_t* out);
/* k-way merge of per-shard results after the all-gather (multi-GPU, one process per GPU):
 * gathered_* are device arrays laid out [n_shards][nq][k] (what ncclAllGather produces from each
 * rank's [nq][k]); out_* are device [nq][k].  Asynchronous on the searcher's stream. */
int mse_merge_topk_dev(mse_searcher* s, const void* gathered_scores_dev, const void* gathered_ids_dev,
                       size_t n_shards, size_t nq, size_t k, void* out_scores_dev, void* out_ids_dev);
/* Same merge for PACKED per-shard blocks: block g = [nq*k] i64 scores then [nq*k] u32 ids, blocks
 * mse_topk_block_bytes(nq, k) apart (what mse_comm_search_dev gathers and mse_shard_group fills). */
size_t mse_topk_block_bytes(size_t nq, size_t k);
int mse_merge_topk_packed_dev(mse_searcher* s, const void* gathered_blocks_dev, size_t n_shards, size_t nq, size_t k,
                              void* out_scores_dev, void* out_ids_dev);
/* Test hook: raw output of the matrix-core scan, out[g][q] = max over rows 32g..32g+31 of the MFMA score of query q
 * (nq <= 256, host arrays), so that tests can measure its distance from the exact-order scores. */
int mse_debug_mfma_group_max(mse_searcher* s, const uint16_t* queries, size_t nq, float* out);
/* Test hook: the selection tournament (the code every search ends in) over keys the caller supplies; host arrays, synchronous.
 * kind: 0 i64, 1 f32, 3 u32.  layout: 0 query-major [nq][n] (nq_pad ignored); 1 element-strided [n][nq_pad]; 2 group-major float
 * [n][nq_pad] as the matrix-core scan writes it (kind 1 only); nq_pad >= nq, columns past nq are never read.
 * ids_out [nq][k]: the k best per query by (key descending, id ascending), padded with 0xFFFFFFFF; keys_out [nq][k]: their raw keys
 * of `kind`, padded with INT64_MIN / -inf / 0; kth_out [nq]: the key the descent leaves behind as a floor for a later select, in the
 * order-preserving unsigned domain (32-bit keys in the top half) -- never above the k-th best key, 0 when fewer than k keys exist.
 * 1 <= k <= 2048; NaN keys are not ordered. */
int mse_debug_select_topk(mse_searcher* s, int kind, int layout, const void* keys, size_t n, size_t nq, size_t nq_pad, size_t k,
                          uint32_t* ids_out, void* keys_out, uint64_t* kth_out);
/* HIP-event timing of the scan kernel (the HBM-bound kernel) on the searcher's stream: returns the
 * totals accumulated so far, then sets the mode: enable 0 = off, 1 = on, 2 = on and reset totals. */
int mse_searcher_scan_timing(mse_searcher* s, int enable, double* total_ms, uint64_t* launches);
/* statistics of the last MFMA-mode call: number of queries whose certificate needed a wider
 * candidate set, and the widest group count used. */
int mse_searcher_last_stats(const mse_searcher* s, uint32_t* n_widened, uint32_t* max_groups);
/* Thresholded group maxima of the 320-query matrix-core pass (unfiltered search, 257 .. 320 queries per pass): a strided sample of
 * the rows gives each query a rigorous threshold, and the scan of the other rows keeps a group maximum only where it exceeds it,
 * in a per-query list, instead of writing a dense array of maxima.  Answers are the same either way.
 * mode 0: auto (used when the base is large enough for two launches to pay and k is small enough for the lists), 1: off,
 * 2: forced (the size rule is skipped, never what correctness needs: a sample of at least k groups).
 * stride: every stride-th 256-row tile is the sample; stride - 1 must be a power of two (3 .. 1025); 0 keeps the current value (33).
 * capacity: survivors kept per query; 0 keeps the current value (8192).  A pass in which a query has more falls back to the dense
 * array: it costs time, never correctness. */
int mse_searcher_set_sparse_maxima(mse_searcher* s, int mode, uint32_t stride, uint32_t capacity);
/* of the last MFMA-mode call: passes that took the thresholded path, how many of them fell back to the dense array (a list
 * overflowed), and the longest survivor list seen (it may exceed the capacity: that is the overflow). */
int mse_searcher_sparse_stats(const mse_searcher* s, uint32_t* passes, uint32_t* fallbacks, uint32_t* longest_list);

/* ---- filtered brute-force search: top-k over an allowed-row set (FAISS SearchParameters.sel / IDSelector) -----------------
 * A filter is one bit per row, kept on the device that was current on the calling thread when it was made, padded with zero bits
 * to whole 256-row scan tiles.  It is immutable: to change one, make another.  It may be shorter than the base it is used on
 * (rows at or past mse_filter_len are excluded -- the flat index grows under add), not longer.  Using it with a base on another
 * device is an error, not a copy.
 * bits: LSB-first bitmap, row r = bit (r % 8) of byte r / 8 (numpy.packbits(..., bitorder="little")); bits past n_rows are ignored.
 * from_ids: duplicates allowed; an id >= n_rows is an error (nothing is made).  Both return NULL on error (mse_last_error). */
typedef struct mse_filter mse_filter;
mse_filter* mse_filter_from_bits(const uint8_t* bits, size_t n_rows);
mse_filter* mse_filter_from_ids(const uint32_t* ids, size_t n_ids, size_t n_rows);
void mse_filter_free(mse_filter* f);
size_t mse_filter_len(const mse_filter* f);      /* n_rows */
size_t mse_filter_count(const mse_filter* f);    /* allowed rows, counted on the device at creation */
/* Brute-force top-k over the allowed rows only.  The result is exactly what mse_bruteforce_topk_f16 returns on a base made of the
 * allowed rows alone, with ids mapped back to the original rows: the same i64 scores, (score desc, id asc) order, unfilled slots
 * INT64_MIN / MSE_ID_NONE.  Arguments and limits are those of the unfiltered calls (k <= 1984); a null filter is an error.
 * MSE_MODE_EXACT scores the filter's allowed rows in the reference order; MSE_MODE_MFMA runs the matrix-core scan with the filter
 * applied in its group maxima (+ exact re-score + certificate); MSE_MODE_AUTO takes the exact path when the allowed rows are few
 * next to the rows (the sparse path), otherwise the unfiltered rule.  MSE_MODE_AUTO host calls of at most one pass go
 * to the base's coalescer, as unfiltered ones do: they share a pass with the requests of the same filter object only. */
int mse_bruteforce_topk_filtered_f16(mse_searcher* s, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k,
                                     int mode, int64_t* scores, uint32_t* ids);
/* The _dev form is asynchronous on the searcher's stream, like mse_bruteforce_topk_f16_dev: the filter (and the buffers) must
 * outlive the work it queued -- synchronise the stream before mse_filter_free. */
int mse_bruteforce_topk_filtered_f16_dev(mse_searcher* s, const mse_filter* f, const void* queries_dev, size_t nq, size_t k,
                                         int mode, uint64_t id_offset, void* scores_dev, void* ids_dev);

/* ---- grouped search: one result per group, collapsed on the device ("collapse" / "grouping search" of other engines) --------------
 * The reference's small-scale server walks its ranked rows and keeps the first frame of each video only (src/main.rs:902-917:
 * `seen_videos.insert(container)` drops every later frame of a container already seen), so that asking for k yields "however many
 * distinct items were among the best k rows".  Here the same step runs on the device and returns k GROUPS.
 * A grouping gives every row a u32 group id.  MSE_GROUP_NONE: the row is a group of its own.  Any other id must be below n_rows (number
 * the groups densely, or use the row id of any member); an id that breaks this is an error at creation and nothing is made.  The array is
 * copied to the device that is current on the calling thread (from_dev: the device the array lives on, which becomes current) and
 * validated and counted there.  A grouping may be SHORTER than the base or index it is used on (rows at or past mse_groups_len are groups
 * of their own -- the flat index grows under add), not longer, and not on another device: the rules of filters.
 * Contract, met bit for bit by every path: for one query order all eligible rows (all rows, or the filter's allowed rows) by the
 * search's own total order -- (score desc, id asc) for the f16 brute force, (distance desc, label asc) for the flat index.  A row is
 * its group's REPRESENTATIVE if no earlier row has the same group.  The answer is the first k representatives with their own scores and
 * ids, padded with INT64_MIN / MSE_ID_NONE (flat index: -FLT_MAX / -1) when fewer than k groups have an eligible row.  So: under a
 * filter a group whose best row is disallowed is represented by its best ALLOWED row; a non-representative is never returned, not even
 * to fill a short list; with every row MSE_GROUP_NONE the answer is the ungrouped answer.
 * How: MSE_MODE_MFMA runs the ordinary (masked) search for k' = max(2k, k + 64) candidates and collapses the ranked
 * list in one workgroup per query; a prefix of the total order collapses to a prefix of the collapsed order, so a query with k
 * representatives -- or a list that came back short -- is answered exactly.  The others go on as a compact set with k' eightfold per
 * round up to the selection limit (1984), and what is still short takes the DENSE path, as every query of MSE_MODE_EXACT does: over all scores of the query the best row of each group
 * by integer atomics (bit-reproducible), every other grouped row out of the ranking, then the ordinary selection.  Dense-path scratch:
 * the exact pass's 8 bytes per query per eligible row, plus 12 bytes (flat index: 8) per query per row of the GROUPING, bounded to 1 GiB
 * per pass by taking fewer than 8 queries per pass once the grouping exceeds 1.1e7 rows.
 * Rows whose own score saturates to INT64_MIN rank last in any case and tie with the rows the dense path takes out of the ranking; it
 * completes a short list from them in id order with one workgroup per query, which is slow and meant for that degenerate case only.
 * (The flat index takes rows out with the all-ones f32 pattern, a NaN below every other key that no dot product produces.) */
#define MSE_GROUP_NONE 0xFFFFFFFFu
typedef struct mse_groups mse_groups;
mse_groups* mse_groups_from_host(const uint32_t* group_of, size_t n_rows);     /* copies; validated on the device */
mse_groups* mse_groups_from_dev(const void* group_of_dev, size_t n_rows);      /* copies */
void   mse_groups_free(mse_groups* g);
size_t mse_groups_len(const mse_groups* g);
size_t mse_groups_count(const mse_groups* g);   /* distinct ids + MSE_GROUP_NONE rows: the most results a search can return */
/* f may be NULL (all rows).  Arguments, modes, limits (k <= 1984), padding and error order as the filtered calls; a null grouping is an
 * error (after the searcher's checks), a grouping that does not fit is one after the filter's.  Groups are looked up by LOCAL row id:
 * id_offset is added only on the way out.  Host calls run on the caller's searcher in every mode (not through the base's coalescer).
 * The _dev form synchronises the searcher's stream (the prefix path decides on the host who goes on); on return the answers are complete. */
int mse_bruteforce_topk_grouped_f16(mse_searcher* s, const mse_groups* g, const mse_filter* f, const uint16_t* queries,
                                    size_t nq, size_t k, int mode, int64_t* scores, uint32_t* ids);
int mse_bruteforce_topk_grouped_f16_dev(mse_searcher* s, const mse_groups* g, const mse_filter* f, const void* queries_dev,
                                        size_t nq, size_t k, int mode, uint64_t id_offset, void* scores_dev, void* ids_dev);
/* of the last grouped call on s: queries answered from the first candidate prefix, from a widened prefix, by the dense path */
int mse_searcher_grouped_stats(const mse_searcher* s, uint32_t out[3]);
/* Measurement hook (scripts/grouped_search_probe.py), as mse_searcher_scan_timing: out (or null) receives the HIP-event milliseconds
 * accumulated by the grouped calls on s while the switch was on -- [0] the collapse kernel of the prefix rounds; of the dense passes
 * [1] the score pass, [2] the group atomics and the demotion, [3] the selection with its collapse -- then sets the switch (0 off, 1 on,
 * 2 on and reset).  While it is on every dense pass ends with a synchronisation. */
int mse_searcher_grouped_timing(mse_searcher* s, int enable, double out[4]);
/* Test hook, like mse_debug_select_topk: the collapse kernel alone over caller-supplied ranked id lists.
 * ids [nq][n_list] best first, MSE_ID_NONE padding at the tail only, n_list <= 2048.  kept_pos [nq][k]: positions in the list of the
 * first k representatives (MSE_ID_NONE padded); n_reps [nq]: representatives in the whole list.  Host arrays, synchronous. */
int mse_debug_collapse_topk(mse_searcher* s, const mse_groups* g, const uint32_t* ids, size_t n_list, size_t nq, size_t k,
                            uint32_t* kept_pos, uint32_t* n_reps);

/* ---- cross-thread query coalescer ----------------------------------------------------------
 * The reference serves ONE query per request from many threads at once: `index.search(&query, k)` under a shared read
 * guard per HTTP request (src/main.rs:896-934,1043-1049), and a thread per core with its own Scratch, one search per
 * request (src/query_disk_index.rs:711-736).  A pass over the rows costs one MI355X the same for 1 query as for 128, so
 * those callers must share passes: mse_dispatcher_topk_f16 may be called from any number of threads; callers block, ONE
 * worker thread (on the device that holds the rows) gathers what is waiting -- until as many queries wait as the last
 * pass answered, or max_queries_per_pass, or the oldest is max_wait_us old -- runs a single pass (matrix-core scan +
 * exact re-score + certificate: the same answers as every mode of mse_bruteforce_topk_f16) and hands each caller its rows.
 * A lone caller never waits for company.  Callers may ask for different k (each gets the first k of the largest k's order);
 * argument errors are returned to their caller without entering the queue, and if a shared pass fails every request of
 * it is repeated alone, so a caller only ever sees its own failure.
 * max_queries_per_pass 0 = 256 (one matrix-core pass); max_wait_us 0 = a tenth of a pass over the rows, 200 us .. 5 ms.
 * mse_bruteforce_topk_f16(..., MSE_MODE_AUTO, ...) goes through a dispatcher the base makes on first use, so the reference's
 * thread-per-core loop coalesces without knowing; mse_index_search does the same inside every mse_index. */
typedef struct mse_dispatcher mse_dispatcher;
mse_dispatcher* mse_dispatcher_new(const mse_base* b, size_t max_queries_per_pass, uint32_t max_wait_us);
void mse_dispatcher_free(mse_dispatcher* d);               /* no call may be in flight */
int mse_dispatcher_topk_f16(mse_dispatcher* d, const uint16_t* queries, size_t nq, size_t k, int64_t* scores, uint32_t* ids);
/* the same over the rows filter f allows (f null: all rows); requests share a pass only with requests of the same filter object */
int mse_dispatcher_topk_filtered_f16(mse_dispatcher* d, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k,
                                     int64_t* scores, uint32_t* ids);
/* out: [0] queries answered, [1] requests, [2] passes, [3] most queries in one pass, [4] passes started by the wait budget,
 * [5] requests repeated alone after a failed shared pass */
int mse_dispatcher_stats(mse_dispatcher* d, uint64_t out[6]);
mse_searcher* mse_dispatcher_searcher(mse_dispatcher* d);   /* the worker's searcher, for scan timing / certificate stats; owned by d */
/* test hook: the next n_passes passes that carry more than one request fail before they start, so that the
 * repeat-each-request-alone path can be exercised (answers must be unaffected) */
int mse_debug_dispatcher_fail_shared(mse_dispatcher* d, uint32_t n_passes);
/* test hook that needs no device (the "not gpu" suite): `threads` host threads x `rounds` one-query requests through the coalescer's
 * queue with a stand-in pass (payload p -> 2 p + 1; payloads divisible by 97 fail, alone).  stats_out as mse_dispatcher_stats;
 * *mismatches = requests that got a wrong answer, a wrong status or no error text. */
int mse_debug_coalescer_selftest(int threads, int rounds, uint32_t max_queries, uint32_t max_wait_us, uint64_t stats_out[6],
                                 uint64_t* mismatches);
/* the same through a coalescer with `workers` worker threads (the graph's request path runs three, csrc/dispatch.h) */
int mse_debug_coalescer_selftest_workers(int threads, int rounds, uint32_t max_queries, uint32_t max_wait_us, int workers,
                                         uint64_t stats_out[6], uint64_t* mismatches);
/* the asynchronous side of the same queue (submit_async / completions), no device needed: async_threads threads keep `window` records
 * each in flight while sync_threads blocking callers share the handle; own_queues != 0: every asynchronous thread has a completion queue
 * of its own and must get back exactly its own records; stats_out[5] = records collected; *mismatches = records handed back twice or
 * never (or to the wrong queue), wrong answers / statuses / error texts */
int mse_debug_coalescer_selftest_async(int async_threads, int window, int n_requests, int sync_threads, uint32_t max_queries, int workers,
                                       int own_queues, uint64_t stats_out[6], uint64_t* mismatches);

/* ---- row-sharded index over the GPUs of one node.  The reference has no multi-GPU
 * code; its query server is a thread per core, each with its own Scratch over shared read-only maps
 * (src/query_disk_index.rs:711-736).  Same shape here with a thread per shard: rows partitioned
 * contiguously (shard g of G holds rows [g*n/G ..), remainder on the first shards), every shard scores
 * the same query batch and returns global ids, the per-shard [nq][k] records meet in ONE buffer on the
 * root device (shard 0's; written over a peer mapping, i.e. xGMI, when the devices allow it) and are
 * merged by (score desc, id asc).  Results equal those of one searcher over all rows.
 * devices[g] = HIP ordinal of shard g (NULL: g mod device count); ordinals may repeat (logical shards). */
typedef struct mse_shard_group mse_shard_group;
mse_shard_group* mse_shard_group_new(const int* devices, size_t n_shards, size_t d);
void mse_shard_group_free(mse_shard_group* g);
size_t mse_shard_group_n_shards(const mse_shard_group* g);
size_t mse_shard_group_len(const mse_shard_group* g);                       /* rows over all shards */
int mse_shard_group_device(const mse_shard_group* g, size_t shard);
int mse_shard_group_peer_mapped(const mse_shard_group* g, size_t shard);    /* 1: writes the gather buffer directly */
mse_searcher* mse_shard_group_searcher(mse_shard_group* g, size_t shard);   /* for scan timing / certificate stats; owned by the group */
/* fill: synthetic rows first_row .. first_row+total_rows made on each shard's device | one host array split
 * over the shards (copied) | one shard borrowed from device memory on that shard's device */
int mse_shard_group_generate(mse_shard_group* g, uint32_t seed, uint64_t first_row, size_t total_rows);
int mse_shard_group_load_host(mse_shard_group* g, const uint16_t* rows, size_t total_rows);
int mse_shard_group_set_shard_device(mse_shard_group* g, size_t shard, const void* rows_dev, size_t n_rows, uint64_t first_row);
/* brute-force top-k over all shards: same contract as mse_bruteforce_topk_f16 (ids are global). */
int mse_shard_group_search(mse_shard_group* g, const uint16_t* queries, size_t nq, size_t k, int mode, int64_t* scores,
                           uint32_t* ids);
/* queries / outputs on the ROOT device (queries complete before the call); returns when the result is complete. */
/* How the per-shard [nq][k] records meet (no reference counterpart: the reference has one address space, src/query_disk_index.rs:711-736).
 * MSE_EXCHANGE_PEER (default): kernels of a shard store its block into the root device's gather buffer through a peer mapping
 * (or one hipMemcpyPeerAsync per shard when the devices cannot map each other); works with several shards per device.
 * MSE_EXCHANGE_RCCL: ONE ncclAllGather of the packed 12-byte records per search among the shards' devices (librccl.so, dlopen'ed),
 * every shard on its own device.  set_exchange returns -1 and leaves the previous exchange in place when RCCL cannot be brought
 * up (shards sharing a device, no librccl, ncclCommInitAll failing): callers degrade, they do not abort. */
#define MSE_EXCHANGE_PEER 0
#define MSE_EXCHANGE_RCCL 1
typedef struct mse_pq mse_pq;         /* (declared in full further down) */
typedef struct mse_codes mse_codes;
typedef struct mse_graph mse_graph;
/* ---- the approximate-search paths over the same shards (rows AND their PQ codes / descriptors / graph) ----
 * A shard's codec, codes (+ descriptor bytes) and graph are ordinary handles made by the caller on the shard's device
 * (mse_set_device(mse_shard_group_device(g, shard)) first) over the shard's rows (mse_shard_group_searcher(g, shard)->base), speaking
 * LOCAL ids; the group adds the shard's first row.  Handles stay the caller's and must outlive their attachment (NULLs detach).
 *   mse_shard_group_pq_scan_topk   mse_pq_scan_topk_batch (ADC top-r, exact fp16 re-score, top-k) over all shards with the answer of the
 *                                  unsharded call bit for bit: (A) every shard's ADC top-r -> exchange -> the index's top-r;
 *                                  (B) every shard re-scores ITS members of it exactly -> exchange -> top-k.  scales: [n_desc] or NULL.
 *   mse_shard_group_query_topk     one graph per shard over its rows (the reference's shards: src/generate_index_shard.rs): every shard
 *                                  answers the batch from its graph (mse_disk_query_topk: its entry table, greedy_search, the k best
 *                                  visited records), ONE exchange, merge by (score desc, id asc) = the merge of the per-shard searches.
 *                                  queries f16 [nq][d] host rows; luts [nq][64*256] (ADC) or NULL with disable_pq; scales [nq][n_desc] or NULL.
 * Both use the group's exchange (peer stores or ONE ncclAllGather of the packed blocks per exchange). */
const mse_base* mse_shard_group_base(const mse_shard_group* g, size_t shard);   /* the shard's rows (owned by the group) */
uint64_t mse_shard_group_first_row(const mse_shard_group* g, size_t shard);
int mse_shard_group_attach_pq(mse_shard_group* g, size_t shard, mse_pq* pq, const mse_codes* codes);
int mse_shard_group_attach_graph(mse_shard_group* g, size_t shard, const mse_graph* graph);
int mse_shard_group_pq_scan_topk(mse_shard_group* g, const float* queries_f32, const float* scales, size_t nq, size_t r, size_t k,
                                 int64_t* scores, uint32_t* ids);
int mse_shard_group_query_topk(mse_shard_group* g, const uint16_t* queries, const float* luts, const float* scales, size_t nq, int disable_pq,
                               size_t beamwidth, size_t search_list, size_t k, int64_t* scores, uint32_t* ids);
int mse_shard_group_set_exchange(mse_shard_group* g, int kind);
int mse_shard_group_exchange(const mse_shard_group* g);
int mse_shard_group_rccl_ranks(const mse_shard_group* g);                   /* ranks as ncclCommCount reports them; 0 = RCCL not up */
/* breakdown of the last search in ms: [0] slowest shard's local search (scan + tournament + re-score + certificate),
 * [1] slowest shard's exchange leg (all-gather / staged copy; ~0 for peer stores), [2] merge on the root, [3] wall clock of the call */
int mse_shard_group_last_timing(mse_shard_group* g, double out_ms[4]);
int mse_shard_group_search_dev(mse_shard_group* g, const void* queries_dev, size_t nq, size_t k, int mode, void* scores_dev,
                               void* ids_dev);

/* One process per GPU instead (the launch shape of torchrun): ONE ncclAllGather of the packed per-shard
 * records over RCCL/xGMI on the searcher's stream, then the same merge on every rank.  RCCL is loaded on
 * first use (librccl.so); the 128-byte id made by rank 0 reaches the other ranks through the host's own
 * rendezvous (any byte transport).  Every rank must call mse_comm_search_dev with the same nq and k. */
typedef struct { char internal[128]; } mse_comm_id;     /* == ncclUniqueId */
typedef struct mse_comm mse_comm;
int mse_comm_unique_id(mse_comm_id* out);
mse_comm* mse_comm_init(const mse_comm_id* id, int rank, int world);  /* collective; on the thread's current device */
void mse_comm_free(mse_comm* c);
int mse_comm_rank(const mse_comm* c);
int mse_comm_size(const mse_comm* c);                   /* rank count as RCCL reports it */
int mse_comm_search_dev(mse_comm* c, mse_searcher* s, const void* queries_dev, size_t nq, size_t k, int mode,
                        uint64_t id_offset, void* scores_dev, void* ids_dev);
/* breakdown of this rank's last mse_comm_search_dev in ms: [0] local search, [1] all-gather (incl. waiting for the slowest rank),
 * [2] merge, [3] their sum; waits for that search to finish */
int mse_comm_last_timing(mse_comm* c, double out_ms[4]);
/* The exchange alone -- this rank's packed block of (score, GLOBAL id) records ([nq*k_in] i64, then [nq*k_in] u32; on its device,
 * complete on the searcher's stream) -> ONE ncclAllGather -> the k best per query of all ranks' records, identical on every rank -- and
 * the two approximate-search paths composed over it, one process per GPU (the protocols of mse_shard_group_pq_scan_topk /
 * _query_topk; first_row = global id of this rank's local row 0; host inputs are the same on every rank; outputs [nq][k] on this
 * rank's device, complete on return). */
int mse_comm_exchange_dev(mse_comm* c, mse_searcher* s, const void* block_dev, size_t nq, size_t k_in, size_t k, void* scores_dev, void* ids_dev);
int mse_comm_pq_scan_topk(mse_comm* c, mse_pq* pq, const mse_codes* codes, mse_searcher* s, const float* queries_f32, const float* scales,
                          size_t nq, size_t r, size_t k, uint64_t first_row, void* scores_dev, void* ids_dev);
int mse_comm_query_topk(mse_comm* c, mse_searcher* s, mse_pq* pq, const mse_codes* codes, const mse_graph* g, const uint16_t* queries,
                        const float* luts, const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k,
                        uint64_t first_row, void* scores_dev, void* ids_dev);

/* ---- flat in-memory index: FAISS IndexScalarQuantizer(QT_fp16, INNER_PRODUCT) as used by
 * src/main.rs:822 (new), :858,:892 (add), :900 (search), :1015,:1053 (ntotal) -------------- */
typedef struct mse_index mse_index;
mse_index* mse_index_new(int d);
void mse_index_free(mse_index* idx);
int mse_index_add(mse_index* idx, const float* x, size_t n);            /* fp32 -> fp16 RNE, appended */
size_t mse_index_ntotal(const mse_index* idx);
/* distances [nq][k] descending, labels [nq][k], -1 where fewer than k vectors exist (:908). */
/* Any number of threads may search at once (the shared `index.read()` of src/main.rs:1046); `add` excludes them (`index.write()`,
 * :1016) and is not starved by them.  Concurrent searches meet in the index's coalescer (above) and share passes: <= 8 waiting
 * queries over a cache-sized index take the exact pass, anything more ONE matrix-core pass + f32 re-score + certificate. */
int mse_index_search(mse_index* idx, const float* queries, size_t nq, size_t k, float* distances, int64_t* labels);
/* mse_index_search over the rows filter f allows: exactly what mse_index_search returns on an index of the allowed rows alone,
 * labels mapped back (same f32 distances; -FLT_MAX / -1 padding).  f may be shorter than the index (made before an add: the new
 * rows are excluded), not longer; a null filter is an error.  Coalesced with the searches of the same filter object. */
int mse_index_search_filtered(mse_index* idx, const mse_filter* f, const float* queries, size_t nq, size_t k,
                              float* distances, int64_t* labels);
/* mse_index_search with one result per group of g (the grouped-search contract above, in the index's order (distance desc, label asc)):
 * the query_index walk of src/main.rs:902-917 on the device.  f may be NULL.  g may be shorter than the index (rows added since are
 * groups of their own), not longer.  Coalesced like every search: requests share a pass when filter AND grouping are the same objects. */
int mse_index_search_grouped(mse_index* idx, const mse_groups* g, const mse_filter* f, const float* queries, size_t nq,
                             size_t k, float* distances, int64_t* labels);
int mse_index_stats(mse_index* idx, uint64_t out[6]);     /* as mse_dispatcher_stats */

/* ---- product quantiser: diskann::vector::ProductQuantizer (vector.rs:308-406) ------------ */
typedef struct mse_pq mse_pq;
mse_pq* mse_pq_load(const float* centroids, size_t n_centroids, const float* transform, size_t n_dims,
                    size_t n_dims_per_code);
void mse_pq_free(mse_pq* pq);
int mse_pq_apply_transform(mse_pq* pq, const float* x, size_t n, float* out);          /* :320-329 */
int mse_pq_quantize_batch(mse_pq* pq, const float* x, size_t n, uint8_t* codes);       /* :331-364 */
int mse_pq_preprocess_query(mse_pq* pq, const float* query, float* lut);               /* :367-384, lut[n_chunks*n_centroids] */
int mse_pq_adc(mse_pq* pq, const float* lut, const uint8_t* codes, size_t n, int64_t* out); /* :387-405 */

/* ---- codec training: diskann/aopq_train.py on the device ----------------------------------------------------------
 * Trains the arrays of opq.msgpack (aopq_train.py:87-93): centroids [n_centroids][n_dims] f32, transform [n_dims][n_dims] f32.  The
 * algorithm is the script's (:33-85) with the expectation over queries taken exactly through their second moment: start from a rotation and
 * per-sub-space max-inner-product k-means; rounds of { Adam steps on the centroids against L = (1/n) sum_x r^T C r, r = x' - y(x'),
 * C = T C0 T^T; one non-parametric OPQ rotation update }.  Adam's moments and step count live in the handle and persist across calls, as
 * the script's one optimiser does (:75).  Rotation and assignment are mse_pq_apply_transform's and mse_pq_quantize_batch's arithmetic.
 * Every sum over rows is an ORDER-FREE SUM: with vmax = max |v| = f 2^ex, f in [0.5, 1) (ex = 0 at vmax = 0) and
 * E = 61 - ceil(log2 n) - ex, each term is llrint((double)v 2^E) (round-half-even), summed in int64 by integer atomics; its value is
 * (double)S 2^-E.  A non-finite term is an error.  Results are the same bits run to run.
 * THE ROTATION SOLVE BELONGS TO THE CALLER: mse_pq_trainer_cross returns M = X'^T Y; the caller computes U S V^T = svd(M) (float64) and
 * passes T_new = (U V^T)^T T_old to mse_pq_trainer_set_transform (:79-85).  This library links no solver.
 * A handle belongs to the device that was current when it was made; calls on one handle must not overlap. */
typedef struct mse_pq_trainer mse_pq_trainer;
/* Shape rules of mse_pq_load; refused before anything is allocated. */
mse_pq_trainer* mse_pq_trainer_new(size_t n_dims, size_t n_dims_per_code, size_t n_centroids);
void mse_pq_trainer_free(mse_pq_trainer* tr);
/* The sample (aopq_train.py:14,70): n host rows, or rows ids[0 .. n) of a resident base, gathered and kept as f16, widened on the device.
 * n < n_centroids and an id at or past the base's rows are errors.  The unrotated sample is kept: every set_transform rotates it afresh. */
int mse_pq_trainer_set_sample_f32(mse_pq_trainer* tr, const float* x, size_t n);
int mse_pq_trainer_set_sample_base(mse_pq_trainer* tr, const mse_base* b, const uint32_t* ids, size_t n);
/* T [n_dims][n_dims] (:69,85): X' = rows of the sample through T, and C = T C0 T^T when a moment is set. */
int mse_pq_trainer_set_transform(mse_pq_trainer* tr, const float* T);
int mse_pq_trainer_set_centroids(mse_pq_trainer* tr, const float* centroids);          /* [n_centroids][n_dims] (:73) */
/* C0 = Q^T Q / m of the UNROTATED queries, [n_dims][n_dims] (:43,51-53 with the mean over queries taken exactly). */
int mse_pq_trainer_set_query_moment(mse_pq_trainer* tr, const float* C0);
/* iters k-means steps: assign; order-free sums of the members' sub-vectors (one vmax over X'); c = (float)(((double)S / (double)count) 2^-E).
 * A cell without members keeps its centroid; *empty_cells (may be NULL) = such cells in the last step, over all sub-spaces. */
int mse_pq_trainer_kmeans(mse_pq_trainer* tr, size_t iters, uint64_t* empty_cells);
/* steps Adam steps (:33-58, torch.optim.Adam's arithmetic in f32): assign; G = R C on the f32-input matrix cores, rows in chunks of 262144;
 * gradient = (float)(sum over chunks of (double)S_c 2^-E_c, times -2 / n) from the order-free sums of G's column blocks by code; update.
 * loss[s] = L at the centroids BEFORE step s's update.  An error without a query moment. */
int mse_pq_trainer_refine(mse_pq_trainer* tr, size_t steps, float lr, float beta1, float beta2, float eps, double* loss);
int mse_pq_trainer_loss(mse_pq_trainer* tr, double* loss);                             /* L now; changes no state */
/* M [n_dims][n_dims] f64 = X'^T Y in the current rotated coordinates (:82-84), through full-width order-free sums of X' by code. */
int mse_pq_trainer_cross(mse_pq_trainer* tr, double* M);
int mse_pq_trainer_read(mse_pq_trainer* tr, float* centroids, float* transform);      /* either may be NULL */
int mse_pq_trainer_codes(mse_pq_trainer* tr, uint8_t* codes);                          /* [n][n_chunks]: the sample under the current state */
/* out [m][n_dims] = rows rows[0 .. m) of X' (the start of :72-73 takes its centroids from sample rows); a row at or past n is an error. */
int mse_pq_trainer_rotated_rows(mse_pq_trainer* tr, const uint32_t* rows, size_t m, float* out);
/* Adam's state out and in (m, v: [n_centroids][n_dims]; t: steps taken), for resuming.  Outputs may be NULL. */
int mse_pq_trainer_adam_state(mse_pq_trainer* tr, float* m, float* v, uint64_t* t);
int mse_pq_trainer_set_adam_state(mse_pq_trainer* tr, const float* m, const float* v, uint64_t t);
/* The gradient the last refine step applied, [n_centroids][n_dims] (zero for cells without members); an error before the first step. */
int mse_pq_trainer_gradient(mse_pq_trainer* tr, float* grad);
/* A loaded quantiser from the current arrays (:87-93); the trainer stays usable. */
mse_pq* mse_pq_trainer_finish(mse_pq_trainer* tr);
/* HIP-event milliseconds of the last step of the last refine call: assignment, residual GEMM, order-free sums of G, Adam. */
int mse_pq_trainer_timing(mse_pq_trainer* tr, float ms[4]);
/* test hooks: the order-free sum alone (host arrays; sums [n_cells][w], *E as defined above); the residual GEMM alone (G [n][n_dims] and
 * l_row [n] = r . G_row for given X', codes [n][n_chunks], centroids and C); the trainer's rows per GEMM pass (default 262144). */
int mse_debug_accumulate_by_code(const float* v, size_t n, size_t w, const uint8_t* code, size_t n_cells, int64_t* sums, int* E);
int mse_debug_residual_gemm(const float* xr, const uint8_t* codes, const float* centroids, const float* C, size_t n, size_t n_dims,
                            size_t n_dims_per_code, size_t n_centroids, float* G, float* lrow);
int mse_debug_pq_trainer_chunk_rows(mse_pq_trainer* tr, size_t rows);

/* ---- shard partition: kmeans.py and the spill-2 assignment of src/dump_processor.rs on the device --------------------
 * Produces what mse_graph_set_entry_centroids, mse_select_shard and the shard files consume: balanced shard centroids (kmeans.py:73-127),
 * the two shards of every row (src/dump_processor.rs:438-461) and, with mse_medioid_ids, each shard's medioid.
 * THE SCORE, defined once: score(x, c) = sum_k (double)x_k (double)c_k, k ascending, one f64 accumulator; x an f16 row widened exactly,
 * c an f32 centroid.  Every product is exact in f64, so a fused and an unfused accumulation give the same bits.  It is the order
 * mse_select_shard states.  Everything below is defined on these f64 values and is the same bits run to run.
 * THE NOISE is the library's generator, not torch.randn (which cannot be reproduced): z(key)[j] = (float)ints(seed, key)[j] * K with ints
 * the integers of mse_base_generate's row `key` and K = (float)(sqrt(3) / 65536): unit variance, bounded at +-3.47 -- not a Gaussian.
 * Keys: initial centroid s: s; the candidate of iteration t >= 1: t S + s; a reroll at iteration t: 2^40 + t S + s.
 * NORMALISATION (torch.nn.functional.normalize, :80,127): ss = sum_k (double)c_k^2, k ascending; norm = 48 Newton steps y = (y + ss / y) / 2
 * from y = 1; c^_k = (float)((double)c_k / norm); a zero row stays zero.
 * FITNESS in integers: sizes[rank][s] = rows whose best (rank 0) / second best (rank 1) normalised centroid is s -- score descending,
 * lowest index on ties -- and F = max over rank, s of |S sizes[rank][s] - n| (S times the script's value, :92-94); worst[rank] = the
 * first s that attains the maximum of that rank.
 * ONE ITERATION t >= 1, temperature T in f32, every operation rounded on its own (:103-122): cand = c + z T; F_new, worst of cand;
 * if F_new < last { c = cand; T *= accept_decay; last = F_new; li = 0 } else { T *= reject_decay; li += 1 };
 * if li > reroll_after { rows worst[0], worst[1] of c = fresh noise; li = 0; T *= reroll_heat; last = F_new }  (the script's quirk, kept);
 * if last 10^6 < n round(stop_fraction 10^6) stop (before the cap; a stop_fraction of 0 never stops); else T = min(temperature_cap, T).
 * Iteration 0 evaluates the initial centroids (:100).  The decision is a one-thread device step; a call enqueues its iterations without
 * a host round trip and polls the stopped flag every 256; once it is set the remaining launches do nothing.
 * A handle is made without touching a device and belongs to the device current at its first device call; calls on one handle must not
 * overlap.  Limits, refused before anything is allocated: 2 <= n_shards <= 64, d % 8 == 0, d <= 4096, n >= n_shards. */
typedef struct mse_partitioner mse_partitioner;
typedef struct mse_partition_config {
    float temperature0, accept_decay, reject_decay, reroll_heat, temperature_cap;   /* 1.0, 0.999, 0.9995, 1.1, 1.5 (:98,108,112,118,122) */
    uint32_t reroll_after;                                                          /* 100 (:114) */
    uint32_t seed;
    double stop_fraction;                                                           /* 0.1 (:120), taken to six decimals */
} mse_partition_config;
typedef struct mse_partition_status {
    uint64_t t;                 /* iterations decided (the initial evaluation not counted) */
    uint64_t last_fitness;      /* F units: S times the script's last_fitness */
    uint64_t last_improvement;
    float temperature;
    uint32_t stopped;
} mse_partition_status;
void mse_partition_config_default(mse_partition_config* cfg);                          /* the script's values, seed 0 */
mse_partitioner* mse_partition_new(size_t n_shards, size_t d, const mse_partition_config* cfg);   /* cfg may be NULL: the defaults */
void mse_partition_free(mse_partitioner* p);
/* The sample (kmeans.py:9): n host rows [n][d] f16, or rows ids[0 .. n) of a resident base gathered on the device.  Resets the annealing. */
int mse_partition_set_sample_f16(mse_partitioner* p, const uint16_t* rows, size_t n);
int mse_partition_set_sample_base(mse_partitioner* p, const mse_base* b, const uint32_t* ids, size_t n);
/* iters more iterations of kmeans.py:102-125 (the first call runs iteration 0 before them); returns early once stopped.  Afterwards the
 * result of :127 and :153 is ready, and the assignment's centroids are that f16 result widened. */
int mse_partition_anneal(mse_partitioner* p, size_t iters);
int mse_partition_state(mse_partitioner* p, mse_partition_status* out);
/* Entry j of the trace belongs to iteration j + 1: F[j] = F_new, code[j] = 0 rejected, 1 accepted, 2 rejected and rerolled. */
int mse_partition_trace(mse_partitioner* p, size_t first, size_t n, uint64_t* F, uint8_t* code);
/* [n_shards][d] each, any may be NULL: the raw centroids, their normalisation (:127), its f16 rounding (RNE: the bytes of centroids.bin). */
int mse_partition_centroids(mse_partitioner* p, float* raw, float* normalised, uint16_t* f16);
/* The assignment's centroids [n_shards][d] f32, used as given: for the reference's result pass the f16 file widened (dump_processor.rs:150-159). */
int mse_partition_set_centroids(mse_partitioner* p, const float* centroids);
/* The two forms of the score pass over the sample against centroids [n_shards][d] given by the caller (they replace nothing in the handle):
 * counting (kmeans.py:82-90) -- sizes [2][n_shards] and, optionally, every row's (best, second) as top2 [n][2] -- and scores out,
 * scores [n][n_shards] f64 (dump_processor.rs:442). */
int mse_partition_count(mse_partitioner* p, const float* centroids, uint64_t* sizes, uint8_t* top2);
int mse_partition_scores(mse_partitioner* p, const float* centroids, double* scores);
/* src/dump_processor.rs:438-461 with --balance-fudge `fudge` (default 0.2, :64): for each row in order and each shard s,
 * key_s = -scale_dot_result_f64(score(x, c_s) - fudge ((double)count_s / (double)bal)); the row goes to the two smallest keys; both
 * counts and bal (which starts at 1) are incremented.  ONE DEVIATION: equal keys go to the lowest shard index (the reference's order then
 * depends on the history of its sort).  Rows are appended to the assignment; counts and bal carry on across calls, so a stream of calls
 * equals one call.  Rows are n host rows, or rows first .. first + n of a resident base.  An error before centroids exist. */
int mse_partition_assign_f16(mse_partitioner* p, const uint16_t* rows, size_t n, double fudge);
int mse_partition_assign_base(mse_partitioner* p, const mse_base* b, size_t first, size_t n, double fudge);
int mse_partition_assign_reset(mse_partitioner* p);                                    /* forget the assignment, counts and bal */
int mse_partition_assignment(mse_partitioner* p, size_t first, size_t n, uint8_t* out);   /* out [n][2]: first choice, second choice */
int mse_partition_counts(mse_partitioner* p, uint64_t* counts, uint64_t* n_assigned);  /* counts [n_shards]; either may be NULL */
/* The assigned rows that belong to shard s, as a filter over rows 0 .. n_assigned, built on the device (mse_filter_from_bits_dev).
 * mse_filter_read_ids gives the shard's member list, ascending: the order dump_processor.rs:452-455 appends them to the shard file. */
mse_filter* mse_partition_shard_filter(mse_partitioner* p, size_t s);
/* HIP-event milliseconds of the last iteration of the last anneal call: candidate + normalisation, counting pass, decision. */
int mse_partition_timing(mse_partitioner* p, float ms[3]);
/* mse_medioid (diskann/src/lib.rs:52-68) over rows[ids] in list order; *id_out = the POSITION in the list (ids may repeat). */
int mse_medioid_ids(const mse_base* b, const uint32_t* ids, size_t n_ids, uint32_t* id_out);
/* test hooks: z(key) (d floats); the normalisation of n_rows rows of d floats (f16_out may be NULL); rows per scores-out pass (65536). */
int mse_debug_partition_noise(uint32_t seed, uint64_t key, size_t d, float* out);
int mse_debug_partition_normalise(const float* c, size_t n_rows, size_t d, float* out, uint16_t* f16_out);
int mse_debug_partition_chunk_rows(mse_partitioner* p, size_t rows);

/* PQ codes (+ optional descriptor bytes) resident in HBM: the mmap'd index.pq-codes.bin /
 * index.descriptor-codes.bin of src/query_disk_index.rs:686-709. */
typedef struct mse_codes mse_codes;
mse_codes* mse_codes_from_host(const uint8_t* codes, size_t n, size_t code_size, const uint8_t* descriptors,
                               size_t n_descriptors);
/* The same from rows already resident in HBM: codes = quantize_batch (vector.rs:331-364) of the f32 widenings of the base's
 * f16 rows -- the encode step of src/dump_processor.rs:468-481 -- computed on the device, 65536 rows at a time; only the
 * descriptor bytes (optional) cross PCIe.  Codes equal mse_pq_quantize_batch's on the same rows. */
mse_codes* mse_codes_quantize_base(mse_pq* pq, const mse_base* b, const uint8_t* descriptors, size_t n_descriptors);
void mse_codes_free(mse_codes* c);
size_t mse_codes_len(const mse_codes* c);
/* out[i] = adc(lut, codes[ids[i]]) + descriptor_product(scales, ids[i])   (query_disk_index.rs:189-203,135-142);
 * scales may be NULL (no descriptor bias). */
int mse_pq_adc_gather(mse_pq* pq, const mse_codes* c, const float* lut, const float* scales, const uint32_t* ids,
                      size_t n_ids, int64_t* out);
/* Full ADC scan of all codes, top-r by approximate score, exact re-score against `base` with the
 * f16 query, final top-k (BASELINE config 5).  base may be NULL: then scores are the ADC scores. */
int mse_pq_scan_topk(mse_pq* pq, const mse_codes* c, mse_searcher* s_or_null, const float* query_f32,
                     const float* scales, size_t r, size_t k, int64_t* scores, uint32_t* ids);
/* The same for nq queries ([nq][n_dims] f32) back to back on one stream with one upload and one download;
 * scores / ids are [nq][k].  The scan keeps one maximum per 64 vectors instead of a score per vector; the r best
 * vectors are then found inside the r best groups (exact, ties by lower id). */
int mse_pq_scan_topk_batch(mse_pq* pq, const mse_codes* c, mse_searcher* s_or_null, const float* queries_f32, size_t nq,
                           const float* scales, size_t r, size_t k, int64_t* scores, uint32_t* ids);
/* A shard's form of the batch call: results as a packed block on the device ([nq*k] i64 scores, [nq*k] u32 ids + id_offset; empty slots
 * INT64_MIN / MSE_ID_NONE), complete on return. */
int mse_pq_scan_topk_block(mse_pq* pq, const mse_codes* c, mse_searcher* s_or_null, const float* queries_f32, size_t nq, const float* scales,
                           size_t r, size_t k, uint64_t id_offset, void* block_dev);
/* Batches of >= 4 queries go through the codes four (12-bit tables) or eight (8-bit tables, batches of >= 8) queries per pass: an
 * integer nomination scan on the matrix cores whose answer is certified against the reference-order re-score of the nominated
 * vectors (csrc/pq.hip); a query whose certificate does not hold is repeated through the exact scan, so results are identical
 * either way.  This counts such repeats in the last batch call.  (A quantiser whose data defeats the 8-bit certificate -- more than
 * an eighth of a batch's eight-per-pass queries repeated -- goes back to four per pass for good.) */
uint32_t mse_pq_last_uncertified(mse_pq* pq);
/* test hook: the group maxima (best ADC score + descriptor bias of every 64 vectors, INT64_MIN past the end) the flat scan
 * nominates with; lut1 == NULL: the one-query kernel, else the two-queries-per-pass kernel.  out0 / out1: [ceil(n/64)] on the host. */
int mse_debug_pq_group_max(mse_pq* pq, const mse_codes* c, const float* lut0, const float* lut1, const float* scales, int64_t* out0,
                           int64_t* out1);
/* HIP-event timing of the four-queries-per-pass scan kernel inside mse_pq_scan_topk_batch (the dominant kernel, for the
 * roofline report): returns the totals accumulated so far, then sets the mode: 0 off, 1 on, 2 on and reset. */
int mse_pq_scan_timing(mse_pq* pq, int enable, double* total_ms, uint64_t* launches);
/* the sustained figure beside it: over the batch calls with at least four scans made while timing was on, *span_ms = time from the
 * first scan's start to the last scan's end, *scans = scans in those spans (back-to-back passes on two streams); reset with timing */
int mse_pq_scan_sustained(mse_pq* pq, double* span_ms, uint64_t* scans);
/* test hook: the integer nomination scan alone, per_pass = 4 (12-bit tables) or 8 (8-bit tables) queries per pass over the codes.
 * luts [per_pass][64*256] (n_valid of them used), scales NULL or [4]; out [per_pass][ceil(n/64)] u32 group maxima of the integer
 * sums, params_out [per_pass][4] = delta, c, eps, ok of each query's table. */
int mse_debug_pq4_group_max(mse_pq* pq, const mse_codes* c, const float* luts, const float* scales, int n_valid, int per_pass,
                            uint32_t* out, double* params_out);
/* ---- the flat scan over an allowed-row set (the post-filter of the reference's query_index, moved into the scan) -----------------
 * Each call returns exactly what its unfiltered form returns on an mse_codes made of the allowed rows alone, in ascending id order, with
 * the ids mapped back (a searcher's base is treated the same way).  The renumbering is monotone, so every (score desc, id asc) order
 * falls the same way.  BOTH stages are filtered: the r best by ADC score (+ descriptor bias) are taken among the allowed rows, then the
 * fp16 exact re-score and the top-k as in the unfiltered call.  Padding is INT64_MIN / MSE_ID_NONE when fewer than k rows are allowed;
 * rows at or past mse_filter_len(f) are excluded.  A null filter, a filter longer than the codes or made on another device than the
 * quantiser, and an unknown mode are errors and write nothing, like r or k out of range; the limits on r, k and nq are those of the
 * unfiltered calls.  The filter must outlive the call.
 *   MSE_PQ_FILTER_SCAN  the pass over all codes with masked group-maximum kernels (csrc/pq.hip): an excluded vector counts like one past
 *                       the end of the codes, a group of 64 without an allowed vector is not loaded at all.  Batches share passes
 *                       (eight, four, two queries) and certify the integer nomination exactly as unfiltered ones do.
 *   MSE_PQ_FILTER_LIST  no scan: the ADC scores of the filter's ascending id list through the gather kernel of mse_pq_adc_gather (same
 *                       arithmetic), then the same select, re-score and top-k; one query at a time.
 *   MSE_PQ_FILTER_AUTO  asks mse_pq_filtered_plan(mse_codes_len(c), mse_filter_count(f), nq) and equals the explicit call at its answer.
 * Results are identical in every mode.  No allowed row: all padding, nothing is launched.  Codec shapes other than 64 x 256 (which have
 * no group-maximum scan) take the LIST path whatever the mode.  One-query calls run directly, not through the quantiser's coalescer.
 * mse_pq_last_uncertified counts the repeats of filtered batch calls too; filtered batches never switch the handle back to four queries
 * per pass (a sparse filter fails certificates for want of allowed vectors, not because of the data). */
#define MSE_PQ_FILTER_AUTO 0
#define MSE_PQ_FILTER_SCAN 1
#define MSE_PQ_FILTER_LIST 2
int mse_pq_scan_topk_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, mse_searcher* s_or_null, const float* query_f32,
                              const float* scales, size_t r, size_t k, int mode, int64_t* scores, uint32_t* ids);
int mse_pq_scan_topk_batch_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, mse_searcher* s_or_null, const float* queries_f32,
                                    size_t nq, const float* scales, size_t r, size_t k, int mode, int64_t* scores, uint32_t* ids);
int mse_pq_scan_topk_block_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, mse_searcher* s_or_null, const float* queries_f32,
                                    size_t nq, const float* scales, size_t r, size_t k, int mode, uint64_t id_offset, void* block_dev);
/* Pure host function: *mode_out = MSE_PQ_FILTER_SCAN or _LIST for nq queries over n_codes rows of which `allowed` pass the filter.  The
 * crossover comes from byte counts plus a fixed cost per LIST query (csrc/api_pq.hip); its two constants were set against one run of
 * scripts/filtered_pq_probe.py and remain provisional.  It is monotone (once LIST is chosen, fewer allowed rows never flip it back) and
 * LIST for allowed = 0.  allowed > n_codes and nq = 0 are errors. */
int mse_pq_filtered_plan(size_t n_codes, size_t allowed, size_t nq, int* mode_out);
/* test hooks: mse_debug_pq_group_max / mse_debug_pq4_group_max through the MASKED kernels -- the maximum over the ALLOWED vectors of each
 * group; a group without one gives INT64_MIN (one and two queries per pass) or the zero-sum key 0 (four and eight). */
int mse_debug_pq_group_max_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* lut0, const float* lut1,
                                    const float* scales, int64_t* out0, int64_t* out1);
int mse_debug_pq4_group_max_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* luts, const float* scales, int n_valid,
                                     int per_pass, uint32_t* out, double* params_out);
/* descriptor_product (src/query_disk_index.rs:135-142) for one id, host-side helper. */
int64_t mse_descriptor_product(const float* scales, size_t n_descriptors, const uint8_t* descriptors, uint32_t id);

/* ---- NeighbourBuffer: diskann/src/lib.rs:74-155 (host) ----------------------------------- */
typedef struct mse_nb mse_nb;
mse_nb* mse_nb_new(size_t cap);
void mse_nb_free(mse_nb* b);
void mse_nb_clear(mse_nb* b);
size_t mse_nb_len(const mse_nb* b);
size_t mse_nb_cap(const mse_nb* b);
void mse_nb_insert(mse_nb* b, uint32_t id, int64_t score);
int mse_nb_next_unvisited(mse_nb* b, uint32_t* id);       /* 1 and *id, or 0 when none */
const uint32_t* mse_nb_ids(const mse_nb* b);
const int64_t* mse_nb_scores(const mse_nb* b);

/* In-RAM Vamana greedy search: diskann::greedy_search (lib.rs:183-211).  Traversal on the host,
 * neighbour scoring on the device (gather-and-score).  adj is [n][max_deg], deg[n].  Results
 * are left in `buf`, best first.  *n_distances receives GreedySearchCounters.distances. */
int mse_greedy_search(mse_searcher* s, const uint32_t* adj, const uint32_t* deg, size_t max_deg, uint32_t start,
                      const uint16_t* query, int base_vectors_only, uint32_t query_breakpoint, mse_nb* buf,
                      size_t* n_distances);

/* Disk-index beam search: query_disk_index::greedy_search (src/query_disk_index.rs:144-212) with the records of
 * index.bin (node.vector = the searcher's base rows, node.vertices = adj/deg, node.url.len() > 0 = has_url, NULL
 * meaning "all"), index.pq-codes.bin and index.descriptor-codes.bin (`c`) resident in HBM.  One batched device
 * submission per beam iteration; traversal on the host in the reference's order, including its quirks (entry
 * point inserted with score 0, :153; the pre-buffer is cleared per beam iteration, not per node, :157).
 * lut = mse_pq_preprocess_query output; scales = DescriptorScales (:463-471) or NULL.  Results: `buf` (best first),
 * the visited list in fetch order (ids + exact scores incl. bias; at most visited_cap written, *n_visited is the
 * full count), *cmps and *pq_cmps = the returned `(cmps, pq_cmps)` (:211). */
int mse_disk_greedy_search(mse_searcher* s, mse_pq* pq, const mse_codes* c, const uint32_t* adj, const uint32_t* deg,
                           size_t max_deg, const uint8_t* has_url, uint32_t start, const uint16_t* query, const float* lut,
                           const float* scales, int disable_pq, size_t beamwidth, mse_nb* buf, uint32_t* visited_ids,
                           int64_t* visited_scores, size_t visited_cap, size_t* n_visited, size_t* cmps, size_t* pq_cmps);
/* The same search, GPU-resident and batched over queries: one workgroup per query keeps the
 * NeighbourBuffer, the pre-buffer and the query's distance table in LDS and the visited sets as bit maps in HBM; no
 * host round trip during a search.  The adjacency lives on the device (mse_graph).  Per query q the outputs equal
 * those of mse_disk_greedy_search: buf_ids/buf_scores [nq][search_list] (first buf_len[q] valid, best first),
 * visited_* [nq][visited_cap] in fetch order, n_visited/cmps/pq_cmps [nq].  starts [nq]; queries [nq][d] f16; luts
 * [nq][64*256]; scales [nq][n_descriptors] or NULL.  Limits: 64 x 256 codec, search_list <= 1024, beamwidth <= 8,
 * max_deg <= 128 (merged indexes carry up to SHARD_SPILL x R neighbours per node, src/dump_processor.rs:282-291). */
/* Called with nq = 1 from many threads at once (the reference's request path: one greedy_search per HTTP request on its own task,
 * src/query_disk_index.rs:436-540,711-736), mse_disk_search_batch / _f32 meet in the graph's coalescer: calls that can share a launch
 * (same vectors, codec, codes, graph, search parameters and kind of inputs) run as ONE batched search, a workgroup per query, and
 * every caller gets exactly what its call returns when made alone. */
typedef struct mse_graph mse_graph;
mse_graph* mse_graph_from_host(const uint32_t* adj, const uint32_t* deg, size_t n, size_t max_deg, const uint8_t* has_url);
void mse_graph_free(mse_graph* g);
int mse_disk_search_batch(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const uint32_t* starts,
                          const uint16_t* queries, const float* luts, const float* scales, size_t nq, int disable_pq,
                          size_t beamwidth, size_t search_list, uint32_t* buf_ids, int64_t* buf_scores, uint32_t* buf_len,
                          uint32_t* visited_ids, int64_t* visited_scores, size_t visited_cap, uint32_t* n_visited,
                          uint32_t* cmps, uint32_t* pq_cmps);
/* The request path in ONE call (src/query_disk_index.rs:436-540 for a batch of queries): entry node, greedy_search, the visited
 * records ordered by exact score and cut to the first k -- nothing but the queries goes up and the k results come down.
 *   mse_graph_set_entries  the entry table: the reference starts a search at the medioid of the shard whose centroid is closest to
 *                          the query (:254-256,447-450); here node_ids name the entry records (shard medioids, or a sample of the
 *                          rows of a one-piece index) and a search starts at the one whose vector has the largest dot product
 *                          with the f16 query (exact top-1 on the device).  Copies of those vectors are kept with the graph.
 *   mse_disk_query_topk    starts == NULL: start nodes by the entry table; otherwise as given.  `queries` ([nq][d] f16) may be a host
 *                          OR a device pointer (embeddings that never left the GPU); everything else is host memory.  luts / scales / disable_pq /
 *                          beamwidth / search_list as mse_disk_search_batch.  ids / scores [nq][k]: the k best visited records by
 *                          (exact score + bias) descending -- equal scores by id ascending (the reference's sort is unstable there) --
 *                          padded with MSE_ID_NONE / INT64_MIN; identical to sorting mse_disk_search_batch's visited list.
 *                          n_visited / cmps / pq_cmps: [nq] or NULL.  Every visited record takes part (no visited_cap to choose).
 *   mse_graph_set_entry_centroids  the reference's entry rule itself (:254-256,447-450): centroids [n_entries][d] f32 are the shard
 *                          centroids of the index header, node_ids the shards' medioids; a search starts at the medioid of the shard
 *                          maximising scale_dot_result_f64(dot(centroid, query)) -- f32 operands (an f16 query widened exactly), the
 *                          sum carried in f64 in index order (as mse_select_shard), the LAST maximum on ties (position_max_by_key).
 *                          Replaces a table set by mse_graph_set_entries and vice versa.  Either setter waits for request-path calls
 *                          in flight and keeps new ones out while it runs.
 *   mse_disk_query_topk_f32  the handler as the reference runs it: f32 queries in (HOST memory); the entry step sees the f32 query, the
 *                          f16 copy (RNE, :477) scores the fetched nodes, preprocess_query (:475) makes the distance tables on the device.
 * THE REFERENCE'S CALL SHAPE (one request = one query on its own task, :436-540,711-736; perf_test.py: 1000 one-query requests at
 * concurrency 100): calls of mse_disk_query_topk(_f32) with nq <= 16 whose queries are host memory meet in the graph's coalescer.
 * Calls that can share a submission (same vectors, codec, codes, graph, disable_pq, beamwidth, search_list, kinds of inputs; k may
 * differ) run as ONE entry step + ONE search launch + ONE select on a searcher owned by the worker thread, and every caller gets
 * exactly what its call returns when made alone.  Such a call only reads `s` for the vectors it names: request threads may share one
 * searcher handle for these calls (4096 request threads do not need 4096 streams).  mse_graph_set_coalescer (before the first such
 * call, or with none in flight): queries per shared submission (0 = 1024), longest wait of the oldest request in microseconds
 * (0 = 200; a lone caller never waits), worker threads (0 = 3: the copies and host side of one submission overlap the kernels of the others).
 * mse_graph_coalescer_stats: {queries, requests, submissions, most queries in one submission, submissions started by the wait
 * budget, microseconds the workers spent executing submissions}.
 * DEVICE-RESIDENT QUERIES: the copy of `queries` runs on the searcher's stream.  If another stream produced them (a tower's), call
 * mse_searcher_wait_stream(s, that_stream) first -- or synchronise that stream -- else the search may read them half written. */
/* WITHOUT A THREAD PER REQUEST (round 5).  The device wants thousands of queries per submission; a sleeping OS thread per request is
 * the wrong vehicle for that (4096 request threads on a 16-core CPU allowance: 25 us of CPU per request just for being woken).  An
 * async host -- the reference serves every connection as a monoio task on a runtime per core (src/query_disk_index.rs:640-655,
 * 716-732) -- keeps its requests in flight as tickets:
 *   mse_disk_query_submit_f32  as mse_disk_query_topk_f32 with nq = 1..16 and entry by the graph's table, but returns as soon as the
 *                          request is queued.  The query (and scales) are copied: the caller's buffers are free at once.  ids / scores
 *                          (/ n_visited / cmps / pq_cmps) are written when the request is executed and must stay valid until its
 *                          ticket has come back.  `user` travels with the ticket (a oneshot sender, a request id).
 *   mse_graph_completions  hands back up to `max` tickets of executed requests of this graph, each exactly once, in completion order;
 *                          sleeps up to timeout_us for the first (0: poll, < 0: no limit).  Returns how many (0: none in time), -1 on
 *                          error.  Any number of threads may submit and collect; a ticket comes back to whichever thread asks next.
 *   mse_completion_queue_* a completion queue of the caller's own.  A host with several event loops -- the reference runs a runtime per
 *                          core -- makes one per loop and passes it as `cq` at submit: those tickets come back through
 *                          mse_completion_queue_wait(q, …) (and its eventfd, mse_completion_queue_fd) and nowhere else, i.e. to the
 *                          loop that submitted them; the shared submissions are the same.  cq = NULL: the graph's own queue
 *                          (mse_graph_completions / mse_graph_completion_fd).  Free a queue only when none of its tickets is out.
 *   mse_graph_completion_fd  an eventfd owned by the graph (valid until its coalescer settings change or it is freed; -1 on error)
 *                          whose counter is bumped once per submission that completed tickets: register it with epoll / io_uring, read
 *                          the 8-byte counter when it fires, then call mse_graph_completions(…, 0) until it returns 0.
 *   mse_ticket_status / _error / _user / _free   0 or the request's error (with its message); the user pointer; release (tickets
 *                          are recycled per thread: a poller that submits and releases on one thread allocates nothing in steady state).
 * Results are those of the synchronous call, bit for bit (the same shared submissions execute both kinds).  Do not free the graph
 * or change its coalescer settings while tickets are out; its entry table may be replaced (a queued request starts from the table
 * that is set when it executes). */
typedef struct mse_ticket mse_ticket;
typedef struct mse_completion_queue mse_completion_queue;
int mse_disk_query_submit_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const float* queries_f32, const float* scales,
                              size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k, uint32_t* ids, int64_t* scores,
                              uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps, void* user, mse_completion_queue* cq,
                              mse_ticket** ticket_out);
/* the same without the copies: queries_f32 (and scales) must stay valid and unchanged until the ticket has come back */
int mse_disk_query_submit_f32_nocopy(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const float* queries_f32,
                                     const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k, uint32_t* ids,
                                     int64_t* scores, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps, void* user, mse_completion_queue* cq,
                                     mse_ticket** ticket_out);
mse_completion_queue* mse_completion_queue_new(void);
void mse_completion_queue_free(mse_completion_queue* q);
int mse_completion_queue_fd(mse_completion_queue* q);
long mse_completion_queue_wait(mse_completion_queue* q, mse_ticket** out, size_t max, long timeout_us);
long mse_graph_completions(const mse_graph* g, mse_ticket** out, size_t max, long timeout_us);
int mse_graph_completion_fd(const mse_graph* g);
int mse_ticket_status(const mse_ticket* t);
const char* mse_ticket_error(const mse_ticket* t);
void* mse_ticket_user(const mse_ticket* t);
void mse_ticket_free(mse_ticket* t);
int mse_graph_set_entries(mse_graph* g, const mse_base* b, const uint32_t* node_ids, size_t n_entries);
int mse_graph_set_entry_centroids(mse_graph* g, const float* centroids, size_t d, const uint32_t* node_ids, size_t n_entries);
int mse_disk_query_topk(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const uint32_t* starts, const uint16_t* queries,
                        const float* luts, const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k,
                        uint32_t* ids, int64_t* scores, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
int mse_disk_query_topk_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const uint32_t* starts, const float* queries_f32,
                            const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k, uint32_t* ids,
                            int64_t* scores, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
/* ---- filtered graph search: the request path over an allowed-row set (the post-filter of the reference's query_index,
 * src/main.rs:904-927, moved into the search) ----
 * The reference has a static form of this: a record whose url is empty is walked through but never returned
 * (src/query_disk_index.rs:172; has_url of mse_graph_from_host).  A filtered search is the reference's greedy_search over an index
 * whose has_url is (has_url AND allowed): three regimes.
 *   MSE_FILTERED_GRAPH  the traversal of src/query_disk_index.rs:144-212 unchanged -- disallowed nodes are fetched, expanded and sit in
 *                       the NeighbourBuffer like any other; a fetched node enters the visited list only if has_url (when the graph has the
 *                       array) AND the filter allows it.  Runs at the caller's search_list.  The entry step is not filtered.
 *   MSE_FILTERED_LIST   no traversal: the exact k best of the rows {allowed AND has_url} by fast_dot(f16 query, row) + descriptor product
 *                       (the bias only with scales and codes that carry descriptors), (score desc, id asc), padding INT64_MIN /
 *                       MSE_ID_NONE; an excluded row is absent, not merely low.  n_visited = cmps = eligible rows, pq_cmps = 0.  f32
 *                       queries are scored through their RNE f16 copies (:477).  pq / luts / starts / beamwidth are not used (beamwidth
 *                       and search_list must still be in range); d must be a multiple of 64.  An error while mse_graph_set_dedup is on
 *                       (the reference de-duplicates in visit order, :482-527; a scan has none) unless the filter allows nothing.
 *   MSE_FILTERED_AUTO   mse_filtered_plan(mse_graph_len, mse_filter_count(f), search_list, dedup on?) picks: no allowed row -> LIST
 *                       (all padding, nothing launched); L' = ceil(search_list * n_rows / allowed) <= 1024 -> GRAPH at
 *                       max(search_list, L') (the search then visits about as many ALLOWED nodes as an unfiltered search at search_list
 *                       visits nodes); else LIST -- or GRAPH at 1024 when de-duplication is on.  A pure host function, so a caller can ask
 *                       what AUTO will do; AUTO then equals the explicit call at its answer.
 * Rows at or past mse_filter_len(f) are excluded; a filter longer than the graph, or on another device than the vectors, is an error, as
 * is a null filter or an unknown regime; argument errors write nothing.  The filter must outlive the call / the ticket.  Everything else
 * -- arguments, limits, outputs, coalescing of small calls -- is that of the unfiltered call each one extends.  Sharing: coalesced calls
 * and tickets whose regime resolves to GRAPH share a submission with every request of equal effective search_list, whatever its filter
 * object, unfiltered requests (traversals at their own search_list) included: the launch reads a filter per query ("a filter per query"
 * below).  LIST requests share only with requests of the same filter object.
 *   mse_disk_search_batch_filtered       extends mse_disk_search_batch (:144-212 with :172 filtered): GRAPH, list form
 *   mse_disk_query_topk_filtered / _f32  extend mse_disk_query_topk / _f32 (:436-540)
 *   mse_disk_query_submit_filtered_f32   extends mse_disk_query_submit_f32 (:640-655,716-732: tickets) */
#define MSE_FILTERED_AUTO 0
#define MSE_FILTERED_GRAPH 1
#define MSE_FILTERED_LIST 2
int mse_filtered_plan(size_t n_rows, size_t allowed, size_t search_list, int dedup_on, int* regime, size_t* search_list_eff);
int mse_disk_search_batch_filtered(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* f, const uint32_t* starts,
                                   const uint16_t* queries, const float* luts, const float* scales, size_t nq, int disable_pq, size_t beamwidth,
                                   size_t search_list, uint32_t* buf_ids, int64_t* buf_scores, uint32_t* buf_len, uint32_t* visited_ids,
                                   int64_t* visited_scores, size_t visited_cap, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
int mse_disk_query_topk_filtered(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* f, int regime,
                                 const uint32_t* starts, const uint16_t* queries, const float* luts, const float* scales, size_t nq, int disable_pq,
                                 size_t beamwidth, size_t search_list, size_t k, uint32_t* ids, int64_t* scores, uint32_t* n_visited, uint32_t* cmps,
                                 uint32_t* pq_cmps);
int mse_disk_query_topk_filtered_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* f, int regime,
                                     const uint32_t* starts, const float* queries_f32, const float* scales, size_t nq, int disable_pq, size_t beamwidth,
                                     size_t search_list, size_t k, uint32_t* ids, int64_t* scores, uint32_t* n_visited, uint32_t* cmps,
                                     uint32_t* pq_cmps);
int mse_disk_query_submit_filtered_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* f, int regime,
                                       const float* queries_f32, const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list,
                                       size_t k, uint32_t* ids, int64_t* scores, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps, void* user,
                                       mse_completion_queue* cq, mse_ticket** ticket_out);
/* ---- grouped graph search: one result per group on the request path (the `seen_videos` walk of the reference's query_index over
 * what the large-scale handler, src/query_disk_index.rs:436-540, visited) ----
 * Contract, met bit for bit by every path.  A grouped request-path call returns, per query, the visited records the ungrouped call would
 * rank -- those that survive the de-duplication when mse_graph_set_dedup is on -- in the same total order (exact score + bias descending,
 * id ascending); a record is kept only if no earlier record in that order has its group; the first k kept records are returned with their
 * own scores, padded with MSE_ID_NONE / INT64_MIN.  In numpy: sort the visited list by (score desc, id asc), keep the first record of
 * every group, take the first k.  Order of steps: de-duplication (visit order, as the reference has it before its sort), then the group
 * step, then the selection.
 * Grouping rules are those of mse_groups: a row of group MSE_GROUP_NONE, or at or past mse_groups_len, is a group of its own; a grouping
 * longer than the graph, or on another device than the vectors, is an error.  A grouping is BY ROW ID: after mse_graph_compact the caller
 * remaps it through old_to_new.  A non-representative is never returned, not even to fill a short list; with every row MSE_GROUP_NONE the
 * answer is the ungrouped answer bit for bit.  n_visited, cmps and pq_cmps are those of the ungrouped call (n_visited counts every visited
 * record): the traversal does not change.
 * This is an APPROXIMATE search: the answer is the collapse of what this search visited at this search_list, not the k best groups of the
 * index.  When one group's rows crowd the visited list fewer than k groups come back, which shows as padding; the caller may ask again
 * with a longer search_list (nothing is widened automatically).
 * With a row filter (f not NULL; f NULL: the unfiltered traversal, regime is ignored):
 *   MSE_FILTERED_GRAPH  the visited list is already filtered and the group step runs over it as above: a group whose best row is
 *                       disallowed is represented by its best allowed VISITED row.
 *   MSE_FILTERED_LIST   the grouped exact answer over the eligible rows {allowed AND has_url}: scores fast_dot + descriptor product (with
 *                       scales and descriptors), order (score desc, id asc), one row per group, counters as LIST.  Scratch: the grouped
 *                       brute force's dense pass (12 bytes per query per row of the grouping, fewer than 8 queries per pass past 1.1e7
 *                       rows).  Still an error while de-duplication is on.
 *   MSE_FILTERED_AUTO   mse_filtered_plan decides as for the filtered call, and the call equals the explicit call at its answer.
 * Validation order: the filtered or unfiltered call's own checks, then "null grouping" (an error of its own), then the grouping's fit;
 * argument errors write nothing.  The grouping must outlive the call / the ticket.  Coalesced calls and tickets share a submission only
 * with requests of the same grouping object (and regime and search_list; filters as for the filtered calls: any in GRAPH, the same object
 * in LIST), never with ungrouped ones; k may differ between sharers.
 * How: one workgroup per query removes every non-best record of a group from the device-resident visited list in place
 * (integer atomics on a hash table in LDS, in global memory for lists past 4096 records) between the de-duplication and the selection:
 * no host decision, no extra synchronisation, no second copy.  The shard's block form has no grouped twin HERE: it is
 * mse_disk_query_topk_block_grouped, declared with the shard group's grouped searches ("grouped search across the shards" below). */
int mse_disk_query_topk_grouped(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_groups* groups, const mse_filter* f,
                                int regime, const uint32_t* starts, const uint16_t* queries, const float* luts, const float* scales, size_t nq,
                                int disable_pq, size_t beamwidth, size_t search_list, size_t k, uint32_t* ids, int64_t* scores, uint32_t* n_visited,
                                uint32_t* cmps, uint32_t* pq_cmps);
int mse_disk_query_topk_grouped_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_groups* groups, const mse_filter* f,
                                    int regime, const uint32_t* starts, const float* queries_f32, const float* scales, size_t nq, int disable_pq,
                                    size_t beamwidth, size_t search_list, size_t k, uint32_t* ids, int64_t* scores, uint32_t* n_visited,
                                    uint32_t* cmps, uint32_t* pq_cmps);
/* the ticket form: mse_disk_query_submit_filtered_f32 with a grouping (f may be NULL) */
int mse_disk_query_submit_grouped_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_groups* groups, const mse_filter* f,
                                      int regime, const float* queries_f32, const float* scales, size_t nq, int disable_pq, size_t beamwidth,
                                      size_t search_list, size_t k, uint32_t* ids, int64_t* scores, uint32_t* n_visited, uint32_t* cmps,
                                      uint32_t* pq_cmps, void* user, mse_completion_queue* cq, mse_ticket** ticket_out);
/* ---- a filter per query: the filtered request path for a batch whose queries each bring their own allowed-row set ----
 * A filter is a property of the request (this user's sources, "not what I have seen"), a launch serves many requests.  Each call below is
 * the twin of a single-filter call with `filters` ([nq] host array of filter handles; an entry may be NULL: that query is unfiltered)
 * where `f` stands, and the two top-k forms take an optional grouping (NULL: ungrouped; one grouping for the call -- it is a property of
 * the index).
 * Contract: for every query i the ids, scores, n_visited, cmps and pq_cmps equal, bit for bit, those of the single-filter call made with
 * query i alone, filters[i], the same regime argument and the same other arguments -- the unfiltered (or grouped unfiltered) call where
 * filters[i] is NULL.
 * `regime` is one argument, resolved per query: under MSE_FILTERED_AUTO each query asks mse_filtered_plan with its own
 * mse_filter_count, so the queries of one call may run in different regimes and at different effective search lists.  The call splits
 * its queries, keeping their order, into classes -- GRAPH queries by effective search_list (unfiltered ones at the caller's), LIST
 * queries by filter object, and the LIST queries whose filter allows nothing (padding, nothing launched) -- and runs each class as ONE
 * launch (the kernel reads query q's bitmap and row bound from a device table) or one list pass; results land at the caller's positions.
 * A call whose queries form one class is one submission over the caller's arrays and, with nq <= 16, is coalesced like its twin; a call
 * of several classes runs them one after the other on `s` (inputs gathered into staging that `s` keeps until mse_searcher_free), and
 * then `s` must not be in use by another thread.  Explicit MSE_FILTERED_GRAPH with a filter that allows nothing still traverses (its
 * twin does, and reports its counters).
 * Validation covers all nq entries before anything is written: a null `filters` array, an unknown regime, and per entry what the
 * single-filter call rejects -- a filter longer than the graph or on another device than the vectors, LIST while mse_graph_set_dedup is
 * on (unless that filter allows nothing) -- with the twin's message followed by " (query i)".  On error the outputs are untouched.
 * The filters must outlive the call.  The answer does not depend on the calls made before it on the same handle.
 *   mse_disk_query_topk_filtered_each / _f32   twins of mse_disk_query_topk_filtered / _f32 (of _grouped / _grouped_f32 with groups)
 *   mse_disk_search_batch_filtered_each        twin of mse_disk_search_batch_filtered: GRAPH, list form, always one launch */
int mse_disk_query_topk_filtered_each(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* const* filters,
                                      int regime, const mse_groups* groups, const uint32_t* starts, const uint16_t* queries, const float* luts,
                                      const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k, uint32_t* ids,
                                      int64_t* scores, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
int mse_disk_query_topk_filtered_each_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* const* filters,
                                          int regime, const mse_groups* groups, const uint32_t* starts, const float* queries_f32,
                                          const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k,
                                          uint32_t* ids, int64_t* scores, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
int mse_disk_search_batch_filtered_each(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* const* filters,
                                        const uint32_t* starts, const uint16_t* queries, const float* luts, const float* scales, size_t nq,
                                        int disable_pq, size_t beamwidth, size_t search_list, uint32_t* buf_ids, int64_t* buf_scores,
                                        uint32_t* buf_len, uint32_t* visited_ids, int64_t* visited_scores, size_t visited_cap, uint32_t* n_visited,
                                        uint32_t* cmps, uint32_t* pq_cmps);
/* Test hook, like mse_debug_collapse_topk: the group step alone over caller-supplied UNRANKED lists.  ids / scores [nq][cap] host arrays
 * (holes (MSE_ID_NONE, INT64_MIN) allowed anywhere), n_visited [nq] (clamped to cap); of every group the best live record by (score desc,
 * id asc) stays, every other record of the group becomes a hole, everything else is written back unchanged.  cap 1..65536; the table is
 * in LDS up to cap 4096 and in global memory beyond, exactly as on the request path.  Synchronous. */
int mse_debug_visited_collapse(mse_searcher* s, const mse_groups* groups, uint32_t* ids, int64_t* scores, size_t cap, const uint32_t* n_visited,
                               size_t nq);
/* A shard's form of the call (multi-GPU, below): the [nq][k] results stay on the device as a packed block -- [nq*k] i64 scores, then
 * [nq*k] u32 ids + id_offset (mse_topk_block_bytes(nq, k) bytes at block_dev) -- ready for the exchange; never coalesced. */
int mse_disk_query_topk_block(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const uint32_t* starts, const uint16_t* queries,
                              const float* luts, const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k,
                              uint64_t id_offset, void* block_dev, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
/* Measurement hook (bench.py's gather roofline for the graph search; no counterpart in the reference): HIP events around every
 * beam_search_kernel launch of this searcher + device totals of what the searches gathered.  enable: 0 off, 1 on, 2 on and reset.
 * out (optional, 8 words, read BEFORE `enable` takes effect): kernel microseconds, launches, queries, rows gathered for an exact score
 * (one 2 x d-byte row gather each: the exactly scored neighbours + the entry point, or -- ADC scoring -- the fetched nodes), nodes
 * fetched (one adjacency list each), neighbours
 * scored by ADC (one 64-byte code gather each), beam iterations, iterations whose inserts ran sequentially (equal scores in play). */
int mse_searcher_beam_timing(mse_searcher* s, int enable, uint64_t out[8]);
/* The handler's runtime de-duplication (src/query_disk_index.rs:482-527, DUPLICATES_THRESHOLD 0.95 :99) INSIDE mse_disk_query_topk(_f32)
 * and its block form: before the visited records are ordered, a record whose vector has a dot product above `threshold` with an ALREADY
 * KEPT record (f32 products of the f16 rows, summed k-ascending as mse_dedup_visited; visit order) is dropped -- for every query of the
 * batch on the device.  0 = off (the default: the k best of ALL visited records).  n_visited still counts every visited record.
 * At most 4096 visited records per query (search lists up to ~2000).  Set while no request-path call is in flight. */
int mse_graph_set_dedup(mse_graph* g, float threshold);
int mse_graph_set_coalescer(mse_graph* g, size_t max_queries_per_pass, uint32_t max_wait_us, int workers);
int mse_graph_coalescer_stats(const mse_graph* g, uint64_t out[6]);
/* What the sharing rule decided, since the graph was made: the workers gather waiting requests into batches (the "submissions" counted
 * above) and split every batch into GROUPS of requests that can share a launch; each group runs as one entry step + one search launch +
 * one select (or one list pass).  out = {groups run, requests in them}: groups == requests means nothing shared a launch. */
int mse_graph_coalescer_groups(const mse_graph* g, uint64_t out[2]);
/* everything `producer_stream` (a hipStream_t) holds at the time of the call completes before anything this searcher's stream is
 * given afterwards starts: an event recorded there, waited for here; no host synchronisation */
int mse_searcher_wait_stream(mse_searcher* s, void* producer_stream);
/* ---- Vamana graph build on the device (diskann/src/lib.rs:183-389, driven by
 * src/generate_index_shard.rs:85-133) ----
 * The graph being built is an mse_graph with max_deg = r (lists of at most r ids, stride r) that stays in HBM
 * between the passes; vectors are the searcher's base rows (base vectors first, then the query vectors of the
 * OOD-DiskANN variant, ids >= query_breakpoint).  The reference leaves two things to chance, and both are
 * arguments here: the insertion order (rng.shuffle, lib.rs:291-292,333-334) and the random initial graph. */
typedef struct mse_build_config {   /* IndexBuildConfig, lib.rs:42-52; defaults generate_index_shard.rs:22-33,85-94 */
    uint64_t r, l, maxc;            /* degree bound (<= 64), search list (<= 1024), candidate cap (<= 1024) */
    int64_t alpha, query_alpha;     /* relaxation factors times 2^16 */
    uint32_t saturate_graph, query_breakpoint;
    uint64_t max_add_per_stitch_iter;
} mse_build_config;
mse_graph* mse_graph_new(size_t n, size_t max_deg);                        /* IndexGraph::empty (lib.rs:22-31) */
int mse_graph_to_host(const mse_graph* g, uint32_t* adj, uint32_t* deg);   /* [n][max_deg], [n] */
size_t mse_graph_len(const mse_graph* g);
size_t mse_graph_max_degree(const mse_graph* g);
/* random_fill_graph (lib.rs:376-389): every list topped up to r distinct uniformly drawn ids (a node may draw
 * itself).  The reference draws from clock-seeded fastrand forks; here draw k of node i is
 * mulhi(philox4x32-10(ctr = (k,0,i,0), key = (seed, 0xF111))[0], n), so a seed names one graph. */
int mse_graph_random_fill(mse_graph* g, uint32_t seed, size_t r);
/* build_graph (lib.rs:287-324) over order[0..n_order): for each point greedy_search from the medioid (:183-211),
 * merge_existing_neighbours (:215-221), robust_prune (:227-285), then the back edges (:311-322).  The reference
 * feeds the points to rayon workers under per-list locks, so its result depends on thread timing; here the points
 * are taken `batch` at a time: the searches and prunes of a batch see the graph as it was before the batch, then the
 * batch's lists are replaced, then the back edges are applied in (position in batch, position in list) order.
 * batch = 1 is exactly the single-threaded loop the reference keeps in comments (:294,297).  One workgroup per point
 * (search list, candidates, prune state in LDS, visited set as a bit map in HBM), one wave per touched list for the
 * back edges.  Every score that orders a list or is compared against is the reference's fast_dot, bit for bit; the
 * candidate-candidate products of the two prunes, which only feed `(alpha * s) >> 16 >= score`, may come from the
 * matrix cores, and then decide only when the comparison holds across their error bound (the exact dot settles the
 * rest), so the graph is the same as with exact products throughout. */
int mse_build_graph(mse_searcher* s, mse_graph* g, const uint32_t* order, size_t n_order, size_t batch, uint32_t medioid,
                    const mse_build_config* cfg);
/* robust_stitch (lib.rs:326-374): query nodes are removed from the base nodes' lists; each base node that pointed
 * at a query receives up to max_add_per_stitch_iter of that query's out-neighbours, best first.  queries_order
 * [n - query_breakpoint] = the shuffled query ids, applied one after another. */
int mse_robust_stitch(mse_searcher* s, mse_graph* g, const uint32_t* queries_order, const mse_build_config* cfg);
/* robust_prune alone (lib.rs:227-285) on a caller-supplied candidate list (scratch.visited_list); neigh has room for
 * cfg->r ids, *n_neigh receives the count.  n_cand is unbounded (the best maxc are kept, :233-234). */
int mse_robust_prune(mse_searcher* s, const uint32_t* cand_ids, const int64_t* cand_scores, size_t n_cand, uint32_t p,
                     const mse_build_config* cfg, uint32_t* neigh, size_t* n_neigh);
/* ---- delete rows and repair the graph on the device (FreshDiskANN's delete consolidation, stated so that it is deterministic) ----
 * D is the delete set, N(x) the list of x AS IT WAS WHEN THE CALL STARTED.
 *  1. A node p not in D is affected if N(p) contains a member of D.  Lists of unaffected live nodes are not touched.
 *  2. The candidate list C of an affected p comes from walking N(p) in list order: an entry v not in D contributes v; an entry v
 *     in D contributes the members of N(v), in list order.  From everything contributed, members of D and p itself are dropped and
 *     only the FIRST occurrence of an id is kept.  Every candidate c is scored fast_dot(row p, row c), the reference's value bit
 *     for bit, as merge_existing_neighbours scores (lib.rs:215-221).
 *  3. The new list of p is robust_prune(p, C, cfg) (lib.rs:227-285) exactly as mse_robust_prune and the build compute it: stable
 *     sort by score, cut to cfg->maxc, the alpha walk, saturate_graph honoured.  An empty C gives an empty list.
 *  4. Every v in D ends with an empty list, has_url = 0 and a set bit in the graph's deleted map; a graph that had no has_url
 *     array gets one, all ones elsewhere.
 *  5. Rows, ids and codes do not move: ids stay stable, nothing is compacted (mse_graph_compact below repacks an index).
 * What follows from the rule:
 *  - every candidate list reads only start-of-call lists, and a live node's list is written only by that node's own work, so the
 *    result does not depend on how the affected nodes are batched;
 *  - deleting D1 and then D2 is NOT the same as deleting the union of D1 and D2;
 *  - a second call with the same D changes nothing;
 *  - after the call the graph is, for every search entry point, indistinguishable from
 *    mse_graph_from_host(repaired adj, deg, has_url AND NOT D).
 * The searcher's base supplies the rows; its length must equal the graph's.  Limits: cfg->r <= mse_graph_max_degree(g) <= 128,
 * cfg->r <= 64, cfg->maxc <= 1024, d as the build requires (cfg->l is not used).  Errors (mse_last_error) that leave the graph
 * untouched: a null filter or config; a filter of another length; a node of the graph's entry table (mse_graph_set_entries /
 * _set_entry_centroids) in D -- the caller moves the entry first; an edge outside the graph.  Like the entry setters, the call waits
 * for the request-path calls in flight on the graph (direct, coalesced, tickets) and keeps new ones out while it runs.  Rows already
 * deleted that appear in D again are ignored and not counted in stats[0].
 * Only the request path is kept out.  The other calls that read or write the graph's lists -- mse_graph_search_batch,
 * mse_build_graph, mse_robust_stitch, mse_graph_to_host, mse_graph_random_fill, the shard group's searches over an attached
 * graph -- do not take part in the lock: the caller must not run them while a delete or a restore runs on the same graph.
 * The call's scratch (the candidate slab of one batch, about 256 MiB at the default batch) stays with the searcher until
 * mse_searcher_free, so that repeated small deletes allocate nothing while they hold the graph. */
/* the set bits of `deleted` (an mse_filter over mse_graph_len(g) rows) name the rows to remove; batch = affected nodes per
 * group of launches (0 = default; the result does not depend on it); stats: [0] rows newly deleted, [1] lists rewritten,
 * [2] largest candidate list, [3] candidate lists longer than cfg->maxc */
int mse_graph_delete_rows(mse_searcher* s, mse_graph* g, const mse_filter* deleted, const mse_build_config* cfg, size_t batch,
                          uint64_t stats[4]);
int mse_graph_deleted(const mse_graph* g, uint8_t* out_or_null /* [n] 0/1 */, size_t* count);
/* give freed slots back: clears the deleted mark and sets has_url = 1 for ids that are deleted (others are an error); their lists
 * stay empty until mse_build_graph is run over them (mse_graph_insert_rows below does all of it -- rows, codes, flags and links -- in
 * one call under the lock) */
int mse_graph_restore_rows(mse_graph* g, const uint32_t* ids, size_t n_ids);
/* ---- insert rows into freed slots of a live graph index (the other direction of the delete above) ----------------------------------
 * One call puts n_rows new vectors into n_rows FREE SLOTS: rows that are marked in the graph's deleted map.  The index does not grow;
 * capacity comes from spare slots (upload the graph, the vectors and the codes with more rows than are live, the spare ones with empty
 * lists; mse_graph_delete_rows over the spare ids marks them -- no list is rewritten -- and they are inserted into later).
 *  1. Validate, before anything changes: no null argument; graph and base of one length; codes_or_null, if given, of the graph's
 *     length, and then pq_or_null given with the base's d and the codes' chunk count (a quantiser without codes is refused too);
 *     descriptors given exactly when the codes carry descriptors; cfg within the limits of mse_build_graph (r equal to the graph's
 *     stride and at most 64, l and maxc at most 1024, d a multiple of 32); every slot in range, marked deleted and named once
 *     (checked on the device against the deleted map); start in range, live and not a slot.  On any of these errors mse_last_error
 *     names the check, and rows, codes, descriptors, flags, lists and the deleted map are bit for bit what they were.
 *  2. Stage: row i goes to base row slots[i]; codes[slots[i]] = the code mse_pq_quantize_batch returns for the f32 widening of row i
 *     (the same launches, over a contiguous staging slab); desc[slots[i]] = descriptors[i].  The base's cached norm bound (the MFMA
 *     certificate's three words) is RAISED to cover the new rows, each contributing exactly what a fresh measurement computes for it,
 *     and never lowered: a bound that is too large is still a bound, and mse_base_rows_changed remains the way to re-measure.  A
 *     bound that was never measured stays unmeasured.  Owned bases (mse_base_from_host, mse_base_generate) and wrapped ones
 *     (mse_base_wrap_device) are both written: memory given to mse_base_wrap_device must be writable by the device.
 *  3. Restore: the deleted mark of each slot is cleared, has_url[slots[i]] = has_url_or_null ? has_url_or_null[i] : 1.
 *  4. Link: exactly mse_build_graph(s, g, order = slots, n_rows, batch, medioid = start, cfg) on the graph as it stands after step 3:
 *     the searches and prunes of a batch see the graph as it was before that batch, then the batch's lists are replaced, then the back
 *     edges are applied in (position in batch, position in list) order.  batch = 0 selects a default (64); the result depends on the
 *     batch exactly as the build's does.
 *  5. Lock: the whole call holds the graph's entry lock exclusively, as mse_graph_delete_rows does: a request-path call (direct,
 *     coalesced or tickets) sees the index wholly before or wholly after the insert.  As with the delete, the calls outside that lock
 *     -- mse_graph_search_batch, mse_build_graph, mse_robust_stitch, mse_graph_to_host, brute-force scans and dispatchers over the same
 *     base, the shard group -- are the caller's to keep out while an insert runs.
 *  6. Afterwards the index is, for every search entry point, indistinguishable from a fresh upload of the new rows, the new codes and
 *     descriptors, the linked adj / deg and the new has_url.
 * stats: [0] rows inserted, [1] batches run.  The call's scratch (a staging slab of at most 16384 rows and the link step's buffers)
 * stays with the searcher until mse_searcher_free, so that repeated small inserts allocate nothing while they hold the graph.
 * Growing n and compacting ids: mse_graph_compact below.  Not covered: the shard group, the on-disk writers, the flat index (mse_index). */
int mse_graph_insert_rows(mse_searcher* s, mse_graph* g, mse_pq* pq_or_null, mse_codes* codes_or_null, const uint32_t* slots, size_t n_rows,
                          const uint16_t* rows_f16 /* host [n_rows][d] */, const uint8_t* descriptors_or_null /* host [n_rows][n_desc] */,
                          const uint8_t* has_url_or_null /* host [n_rows] */, uint32_t start, const mse_build_config* cfg, size_t batch,
                          uint64_t stats[2]);
/* the same with the rows already resident on the searcher's device (e.g. an encoder's f16 output), 16-byte aligned; slots, descriptors
 * and flags stay host arrays */
int mse_graph_insert_rows_dev(mse_searcher* s, mse_graph* g, mse_pq* pq_or_null, mse_codes* codes_or_null, const uint32_t* slots, size_t n_rows,
                              const void* rows_f16_dev, const uint8_t* descriptors_or_null, const uint8_t* has_url_or_null, uint32_t start,
                              const mse_build_config* cfg, size_t batch, uint64_t stats[2]);
/* ---- compact deleted rows away and grow capacity on the device ---------------------------------------------------------------------
 * One call repacks a live index into a FRESH (base, codes, graph) triple of `capacity` rows, wholly on the device and out of place: the
 * old handles are only read, everything that holds pointers into them (searchers, dispatchers, coalescer workers, shard groups) goes on
 * working, and the caller swaps handles when it is ready and frees the old ones.  capacity = the live count compacts; capacity above the
 * old length grows.  MEMORY PEAK: the old and the new index are resident together until the caller frees the old one.
 *  1. n = mse_graph_len(g); a row is LIVE when its bit in the graph's deleted map is clear (a graph that was never deleted from: every
 *     row).  Only the deleted map decides: a row with has_url = 0 is live.  s->base must be the rows the graph indexes: n rows, on the
 *     graph's device, d a multiple of 8.  codes_or_null, if given, has n entries; codes_out is null exactly when codes_or_null is.
 *  2. Live rows get the new ids 0 .. n_live - 1 in ascending order of their old ids: the renumbering is monotone, so every
 *     (score desc, id asc) order falls the same way before and after.
 *  3. Base: an owned base of `capacity` rows, row new = row old bit for bit, rows n_live .. capacity - 1 zero; its norm bound is
 *     unmeasured (first use measures it, as for any upload).  Codes: `capacity` entries of the same code_size and n_desc, code and
 *     descriptor bytes copied, the spare tail zero.
 *  4. Graph: the same max_deg; the list of `new` is the list of `old` with every entry sent through the map, order and length
 *     unchanged; entries at or past the length are 0, as mse_graph_new leaves an entry that was never written.  has_url is copied; a
 *     graph that had none gets one (all ones for live rows) only when there is a spare tail.  The spare tail has empty lists,
 *     has_url = 0 and set bits in the new deleted map, so mse_graph_deleted counts capacity - n_live and mse_graph_insert_rows accepts
 *     those slots at once; without a spare tail the new graph has no deleted map, like a fresh upload.  The entry table, the dedup
 *     threshold and the coalescer settings are NOT carried over: the caller sets them on the new graph, node ids through old_to_new.
 *  5. old_to_new [n] (or null): the new id of each old row, 0xFFFFFFFF for a deleted one.  new_to_old [capacity] (or null): the old id
 *     of each new row, 0xFFFFFFFF for a spare slot.  stats_out (or null): [0] n_live, [1] capacity, [2] list entries rewritten,
 *     [3] bytes of rows moved = n_live x (2 d + code_size + n_desc).
 *  6. Errors (mse_last_error names the check): a null s, g, base_out or graph_out, or codes and codes_out not given together;
 *     capacity 0, below n_live or above 2^32 - 2; codes of another length; a base of another length or device; a live list that names
 *     a deleted row or a row >= n (checked on the device before anything is handed back); an allocation failure (the message gives the
 *     bytes asked for and the free device memory).  On any error nothing is returned, nothing is leaked, the out pointers are not
 *     written and the old handles are bit for bit what they were.
 *  7. Lock: the call holds the old graph's entry lock SHARED for its whole time on the device: mse_graph_delete_rows,
 *     mse_graph_restore_rows and mse_graph_insert_rows on the old graph happen wholly before or wholly after it, request-path calls on
 *     the old graph run beside it.  The calls outside that lock (mse_build_graph, mse_robust_stitch, mse_graph_random_fill, writes to a
 *     wrapped base) are the caller's to keep out.  Everything runs on s's stream; the call returns with that stream drained.
 * Not covered: an in-place variant (for an index above half of the device memory), the shard group, the on-disk writers, the flat
 * index (mse_index). */
int mse_graph_compact(mse_searcher* s, const mse_graph* g, const mse_codes* codes_or_null, size_t capacity, mse_base** base_out,
                      mse_codes** codes_out, mse_graph** graph_out, uint32_t* old_to_new, uint32_t* new_to_old, uint64_t stats_out[4]);
/* The live rows of a graph as a row filter, so that the flat scans (mse_pq_scan_topk*_filtered, mse_bruteforce_topk_filtered_f16,
 * mse_index_search_filtered) can serve a mutated index without compacting it.  Returns a fresh, immutable filter over mse_graph_len(g)
 * rows (free it with mse_filter_free): a bit is set where the row is NOT in the graph's deleted map and -- with and_has_url != 0 and a
 * has_url array present -- has_url != 0.  Built on the device; it is a SNAPSHOT, taken with the graph's entry lock held shared (as
 * mse_graph_compact reads the graph): later deletes, restores and inserts need a new filter.  A graph that was never deleted from gives
 * an all-ones filter.  NULL on error. */
mse_filter* mse_graph_live_filter(const mse_graph* g, int and_has_url);

/* ---- row filters as values: set algebra, predicates over resident data, read-back (FAISS IDSelectorAnd/Or/XOr/Not, range_search) ----
 * Every creator below builds its result on the device and returns a FRESH immutable filter -- bitmap padded with zero words to whole
 * 256-row tiles, ascending id list, count -- or NULL with mse_last_error, and then has made nothing.  Operands are never modified and
 * may be freed at once afterwards.  Creators block until the filter is complete.  mse_filter_from_scores runs on the searcher's stream
 * and uses its scratch (one call per searcher at a time); the others use the null stream, like mse_filter_from_ids.
 * Lengths: a filter reads as zeros at and past its own mse_filter_len (the rule of the searches).  No result has a set bit at or past
 * its own length.  Devices: operands made on different devices are an error, not a copy; a result lives with its operands (from_descriptors:
 * where the codes' descriptor bytes live; from_scores: on the base's device; from_bits_dev: where the bits live), and that device is the
 * calling thread's current device afterwards, as after mse_graph_live_filter.
 * Memory: these creators size the id list by the count (count pass, then write pass): a result holds n_rows / 8 bytes of bitmap and
 * 4 x count bytes of ids.  (mse_filter_from_bits / _from_ids / mse_graph_live_filter keep n_rows x 4 bytes of id list whatever the count.)
 *   mse_filter_combine           a OP b over max(len a, len b) rows; the shorter operand reads as zeros.  An op outside 0..3 is an error.
 *   mse_filter_not               NOT a over n_rows rows (0 = mse_filter_len(a)); n_rows < mse_filter_len(a) is an error; the rows in
 *                                [len a, n_rows) come out allowed.
 *   mse_filter_from_descriptors  over mse_codes_len(c) rows: bit r is set iff lo[j] <= desc[r][j] <= hi[j] for EVERY channel j of the
 *                                codes' n_descriptors (lo, hi: host arrays of that many bytes, inclusive; lo[j] > hi[j] allows nothing).
 *                                Reads the descriptor bytes as they are on the device now (after mse_graph_insert_rows: the new rows').
 *                                Codes without descriptor bytes, or with more than 8 per row, are an error.
 *   mse_filter_from_scores       over mse_base_len rows: bit r is set iff fast_dot(row r, query) >= threshold -- the reference-order i64
 *                                score, exactly what mse_bruteforce_scores_f16 returns (saturation and NaN as there: threshold INT64_MIN
 *                                allows every row) -- AND, with `within`, r is allowed by it.  `within` must be on the base's device and not
 *                                longer than the base.  Widths: those of mse_bruteforce_scores_f16.  A null query is an error.
 *   mse_filter_from_bits_dev     mse_filter_from_bits of a bitmap that is already in device memory ((n_rows + 7) / 8 bytes, same layout;
 *                                bits past n_rows are ignored).  Host memory is an error.
 * Read-back (blocking; both return non-zero and write nothing on error):
 *   mse_filter_to_bits           writes exactly (mse_filter_len(f) + 7) / 8 bytes in the from_bits layout; a null buffer is an error.
 *   mse_filter_read_ids          the allowed ids number first .. first + n of the ascending list; first + n > mse_filter_count(f) is an
 *                                error. */
#define MSE_FILTER_AND    0   /* a & b  */
#define MSE_FILTER_OR     1   /* a | b  */
#define MSE_FILTER_XOR    2   /* a ^ b  */
#define MSE_FILTER_ANDNOT 3   /* a & ~b */
mse_filter* mse_filter_combine(const mse_filter* a, const mse_filter* b, int op);
mse_filter* mse_filter_not(const mse_filter* a, size_t n_rows);
mse_filter* mse_filter_from_descriptors(const mse_codes* c, const uint8_t* lo, const uint8_t* hi);
mse_filter* mse_filter_from_scores(mse_searcher* s, const uint16_t* query_f16, int64_t threshold, const mse_filter* within_or_null);
mse_filter* mse_filter_from_bits_dev(const void* bits_dev, size_t n_rows);
int mse_filter_to_bits(const mse_filter* f, uint8_t* bits);
int mse_filter_read_ids(const mse_filter* f, size_t first, size_t n, uint32_t* out);
/* measurement hook of the creators above (for scripts/filter_ops_probe.py): *last_ms (or null) receives the HIP-event time of the kernel
 * that wrote the bitmap in the last creator call made while the switch was on -- the combine / descriptor / threshold kernel alone (for
 * from_bits_dev: clear, copy and tail mask), without the count and write passes and without from_scores' scan -- then the switch is set
 * (0 off, 1 on, 2 on and reset).  Process-wide; while it is on every creator call waits for its kernel once more. */
int mse_filter_kernel_timing(int enable, double* last_ms);
/* ---- row filters across shards: a filter over GLOBAL row ids cut into per-shard filters over LOCAL ids on the device, and back -------
 * (no reference counterpart: the reference post-filters one address space, src/query_disk_index.rs:172.)  Both creators follow the rules
 * of the creators above -- fresh immutable filter, id list sized by the count, NULL with mse_last_error and nothing made on error, null
 * stream, blocking -- except that the calling thread's current device is the same after the call as before it.
 *   mse_filter_slice   over n_rows LOCAL rows: bit r = bit first_row + r of f, zero where that is at or past mse_filter_len(f).  The rule
 *                      per word: out[w] = funnel(in[w0 + w], in[w0 + w + 1]) >> (first_row & 31), w0 = first_row >> 5, masked to n_rows;
 *                      first_row need not be a multiple of 32 (2 999 rows over 4 shards start at 750, 1 500 and 2 250).  device: where
 *                      the result lives, -1 = f's device; for another device the word range the slice reads goes over by ONE peer copy
 *                      and is sliced there.  n_rows = 0 and a null filter are errors.
 *   mse_filter_concat  the inverse, over n_rows GLOBAL rows: part i occupies rows [first_rows[i], first_rows[i] + mse_filter_len(parts[i]));
 *                      rows no part covers read as zero.  Parts that overlap, a part that reaches past n_rows, a null part and n_rows = 0
 *                      are errors; parts may come in any order and may share a boundary word.  device: -1 = the first part's device; a
 *                      part on another device comes over by one peer copy of its words. */
mse_filter* mse_filter_slice(const mse_filter* f, uint64_t first_row, size_t n_rows, int device);
mse_filter* mse_filter_concat(const mse_filter* const* parts, const uint64_t* first_rows, size_t n_parts, size_t n_rows, int device);

/* ---- near-duplicate join: exact pairs of a resident base, keep-first groups ------------------------------------------------------------
 * The reference meets its near-duplicates twice.  At ingest, -D (src/dump_processor.rs:375-392) hashes a 64-bit binarisation of each
 * embedding into a ring of the last 2^21 records ("distance thresholding is too costly to do over a long range so just do it badly").
 * At query time the handler multiplies the visited vectors against themselves and retains a record only if no already retained one
 * lies above DUPLICATES_THRESHOLD (src/query_disk_index.rs:99,513-527) -- mse_graph_set_dedup / mse_dedup_visited here.  The join below
 * is the ingest half done exactly: the pairs are found by a Gram matrix on the matrix cores and confirmed in reference order.
 *
 * mse_join_self returns ALL pairs (lo, hi) of rows of the searcher's base with lo < hi, hi - lo <= window (window 0: no limit), both rows
 * allowed by within_or_null when one is given, and fast_dot(row lo, row hi) >= threshold -- the reference-order i64 score, the number
 * mse_bruteforce_scores_f16 returns with one of the rows as the query (fast_dot is symmetric; saturation and NaN as there).  The test is
 * >=, as in mse_filter_from_scores; the handler's test is > on f32 sums, so a caller who wants strictness passes threshold + 1.  Each
 * pair carries its exact score.  Canonical order: hi ascending, then lo ascending.  The list lives on the base's device and is
 * immutable; its bytes do not depend on the run, the mode, the size of the internal candidate buffer or the calls made before on the
 * same searcher.
 * Modes (MSE_MODE_*): EXACT scores every pair of the schedule on the vector ALU in reference order.  MFMA runs 128 x 128 Gram tiles of
 * the lower triangle that meet the window band on the f16 matrix cores (tiles whose rows `within` excludes altogether do no work), an
 * accumulator nominates a pair when it is >= threshold - bound (bound: 2.8e-4 x the largest row norm squared plus the subnormal term,
 * the brute-force certificate's allowance), and every nominated pair is re-scored in reference order; when no bound can be stated (a
 * width that is no multiple of 64, a non-finite row) the exact path runs.  AUTO is MFMA.  A full candidate buffer makes the strip of
 * tiles run again in windows of its nominations; the answer is the same.
 * The call runs on the searcher's stream, uses the searcher's scratch (one call per searcher at a time) and blocks until the list is
 * complete.  More than max_pairs pairs: an error that makes nothing; mse_join_stats then holds the true count in [3].
 * Errors, in this order: a null searcher; a `within` longer than the base or made on another device (the messages of the filtered
 * searches); an unknown mode.  A base of 0 rows gives an empty list.  A graph's base: pass mse_graph_live_filter(g, 0) as `within` --
 * deleted slots hold stale rows -- and keep deletes, inserts and restores on that graph out while the call runs, as for any brute-force
 * scan over a graph's base (the lock notes of mse_graph_delete_rows / mse_graph_insert_rows).
 *   mse_pairs_rows / _count   rows of the base the list was made over | pairs
 *   mse_pairs_read            pairs first .. first + n of the canonical order (any output may be null); past the count is an error
 *   mse_join_stats            of the last join on s (mse_join_self, or mse_join_cross below): [0] tiles that did work, [1] pairs nominated, [2] pairs re-scored,
 *                             [3] pairs kept (or the count that did not fit), [4] strip launches repeated for a full buffer,
 *                             [5] rounds of the last keep-first resolution (or mse_pairs_admit) of a list made by s
 *   mse_join_timing           measurement hook (scripts/near_duplicate_probe.py): out (or null) receives the HIP-event milliseconds of the
 *                             last mse_join_self on s -- [0] tile launches, [1] re-score launches, [2] building the list in canonical
 *                             order -- then the switch is set; while it is on the call waits once more per launch
 *   mse_debug_join_candidate_capacity   test hook: nominated pairs one launch may store (0: the default, 2^20)
 * Keep-first over the list (the handler's retain loop applied in row order to the whole base): row i is KEPT iff no kept row j < i forms
 * a pair with it -- the lexicographically first maximal independent set of the pair graph; rep[i] = i for a kept row, the lowest kept
 * earlier neighbour for a dropped one.  Rows `within` excluded are in no pair: kept and ungrouped.  Resolved on the device in rounds
 * over integer state (dropped as soon as one earlier neighbour is kept, kept once all are dropped; a chain of m pairs takes about m
 * rounds), once per list, on the null stream; the result is bit-reproducible.
 *   mse_pairs_duplicates        the dropped rows as a fresh filter, ready for mse_graph_delete_rows
 *   mse_pairs_groups            a fresh grouping: label rep[i] for every row of a group of two or more (the representative included),
 *                               MSE_GROUP_NONE for every other row; every member scores >= threshold against its representative
 *   mse_pairs_representatives   rep, mse_pairs_rows(p) entries, to the host
 * Not covered: connected-component grouping, the shard group. */
typedef struct mse_pairs mse_pairs;
mse_pairs* mse_join_self(mse_searcher* s, int64_t threshold, uint64_t window, const mse_filter* within_or_null, int mode, uint64_t max_pairs);
void mse_pairs_free(mse_pairs* p);
size_t mse_pairs_rows(const mse_pairs* p);
size_t mse_pairs_count(const mse_pairs* p);
int mse_pairs_read(const mse_pairs* p, size_t first, size_t n, uint32_t* lo, uint32_t* hi, int64_t* scores);
int mse_join_stats(const mse_searcher* s, uint64_t out[6]);
int mse_join_timing(mse_searcher* s, int enable, double out[3]);
int mse_debug_join_candidate_capacity(mse_searcher* s, uint64_t n);
mse_filter* mse_pairs_duplicates(const mse_pairs* p);
mse_groups* mse_pairs_groups(const mse_pairs* p);
int mse_pairs_representatives(const mse_pairs* p, uint32_t* rep);
/* ---- cross join: near-duplicates of incoming rows against a resident base, admission, select ----------------------------------------
 * The self-join cleans an index that is dirty; this keeps a live one clean.  It is the exact form of the reference's ingest step -D
 * (src/dump_processor.rs:375-392, a 64-bit binarisation hashed into a ring of the last 2^21 records).
 *
 * mse_join_cross: s searches the resident base B (n rows); `incoming` is a second base Q (m rows; mse_base_from_host, or
 * mse_base_wrap_device over an encoder's f16 output) of the same width on the same device.  The result is EVERY pair (b, j) with b a row
 * of B that within_or_null allows (when given), j a row of Q, and fast_dot(B[b], Q[j]) >= threshold -- the reference-order i64 score,
 * the number mse_bruteforce_scores_f16 returns with Q[j] as the query; >=, saturation and NaN as for mse_join_self.
 * The list is an mse_pairs of kind 1: a CSR over the incoming row j, which takes the hi role because it comes later in ingest order;
 * within each j the base ids ascend, each with its exact score.  mse_pairs_read returns lo = base row, hi = incoming row in canonical
 * order (hi ascending, then lo ascending); mse_pairs_rows is m.  There is no window: the two id spaces are unrelated.
 *   mse_pairs_kind        0 for a self list, 1 for a cross list
 *   mse_pairs_base_rows   n for a cross list, mse_pairs_rows for a self list
 * mse_pairs_duplicates, _groups and _representatives on a cross list are errors that name mse_pairs_admit.
 * The list's bytes do not depend on the run, the mode, the candidate buffer's size (mse_debug_join_candidate_capacity applies), earlier
 * calls on s, whether Q was copied from the host or wrapped, or how the batch is cut: the list of rows [a, c) of Q given alone is the
 * slice of the whole list with hi shifted by a.
 * Modes as for mse_join_self.  EXACT scores every pair of the rectangle on the vector ALU in reference order.  MFMA and AUTO run 128 x 128
 * tiles of the m x n rectangle on the f16 matrix cores and nominate by accumulator * 2^32 >= threshold - bound; every nomination is
 * re-scored in reference order.  The bound is stated for a pair with one row from each base: the one-base formula of mse_join_self over
 * the element-wise maximum of the two bases' three norm figures (largest row norm, largest subnormal mass of a row, largest component);
 * |a||b| <= max^2, and the subnormal term is monotone in both of its figures.  MSE_GRAM_EPS_SCALE applies.  Where no bound can be stated
 * -- a non-finite component in either base -- the exact tiles run whatever mode was asked for.
 * Schedule: a strip is a run of base tiles by all incoming tiles (incoming fastest), so workgroups that are resident together share a
 * base tile and the base streams from HBM once per strip; strips are cut along the incoming side too when m / 128 exceeds a strip.  The
 * strip rule (one reservation per tile, windows of the scanned tile numbering when the buffer overflows), the data-only rank inside a
 * tile and "a tile whose base rows `within` excludes altogether loads nothing" are the self-join's.
 * mse_join_stats and mse_join_timing of s describe the last join on s, self or cross, with the same meaning per field.
 * Errors, in this order: a null searcher or a null incoming base; a width or device mismatch between the two bases; the `within` errors
 * of the filtered searches; an unknown mode.  m = 0 or n = 0 gives an empty list over m rows.  More than max_pairs pairs: an error that
 * makes nothing and leaves the true count in stats [3].  A graph's base: pass mse_graph_live_filter(g, 0) as `within`, and keep deletes,
 * inserts and restores on that graph out while the call runs, as for mse_join_self.
 *
 * mse_pairs_admit: keep-first continued from the index into the batch.  `among_or_null` is an ordinary self list over the same m incoming
 * rows (mse_join_self on a searcher over Q).  The rule is the handler's retain loop (src/query_disk_index.rs:513-527) run over "allowed
 * base rows first, all retained, then the batch in row order": incoming row j is KEPT iff it has no cross pair and no kept incoming row
 * j' < j pairs with it in `among`.  A row dropped by the base is dropped and therefore drops nobody: with b ~ j1 ~ j2 and b !~ j2, j1 goes
 * and j2 stays.  rep_base[j] (m entries, or null) is j's lowest base partner, 0xFFFFFFFF when it has none; rep_incoming[j] (m entries, or
 * null) is j itself when j is kept, its lowest kept earlier `among` neighbour when that is what dropped it, 0xFFFFFFFF when the base
 * dropped it.  *kept_out is a fresh filter over m rows, on the device.  Resolved on the device in the integer rounds of the self list,
 * started from a state in which rows with a cross pair are already dropped; bit-reproducible; no label crosses to the host before the
 * outputs.  among = null: only the base decides.  The rounds it took are left in mse_join_stats [5] of the searcher that made `cross`.
 * Errors: `cross` is not a cross list; `among` is not a self list; the row counts or devices differ; kept_out is null.
 *
 * mse_base_select: a fresh owned base holding the rows of b that `keep` allows, in ascending order -- a 16-byte-vector row gather on the
 * device.  With it an encoder's device output flows wrap -> cross join -> admit -> select -> mse_graph_insert_rows_dev without its rows
 * crossing PCIe.  A filter longer than the base or on another device is an error; a count of 0 gives a base of 0 rows.
 * Not covered: the shard group, connected-component grouping, an approximate join through the graph, PQ-code pre-filters. */
mse_pairs* mse_join_cross(mse_searcher* s, const mse_base* incoming, int64_t threshold, const mse_filter* within_or_null, int mode,
                          uint64_t max_pairs);
int mse_pairs_kind(const mse_pairs* p);
size_t mse_pairs_base_rows(const mse_pairs* p);
int mse_pairs_admit(const mse_pairs* cross, const mse_pairs* among_or_null, mse_filter** kept_out, uint32_t* rep_base, uint32_t* rep_incoming);
mse_base* mse_base_select(const mse_base* b, const mse_filter* keep);
/* mse_shard_filter: one LOCAL filter per shard of a group, each on its shard's device -- what the filtered searches of the group take.
 *   mse_shard_group_filter             mse_filter_slice of `global` at each shard's first row and length.  A filter shorter than the group
 *                                      excludes the rows past it; one longer than max(first row + rows) over the shards is an error.
 *   mse_shard_group_filter_from_local  a copy of per_shard[g] for every shard g; each must have its shard's length and device.
 *   mse_shard_group_live_filter        mse_graph_live_filter(graph, and_has_url) of every shard's attached graph: the rows that deletes
 *                                      through the shards' graphs have left.  A shard without a graph is an error.
 *   mse_shard_filter_count             allowed rows, summed over the shards;  _n_shards: its parts
 *   mse_shard_filter_shard             shard g's local filter, BORROWED (it lives as long as the shard filter)
 *   mse_shard_filter_global            mse_filter_concat of the parts at their first rows over max(first row + rows) rows on `device`
 *                                      (-1: shard 0's): a fresh mse_filter, the caller's to free
 * A shard filter remembers the layout it was made for: every call that re-fills a shard (mse_shard_group_generate, _load_host,
 * _set_shard_device) starts a new layout, and a shard filter of an older layout -- or of another group -- is refused by every call that
 * takes one.  It is immutable, holds no reference to the group, and must outlive the calls it is passed to.
 * The filtered searches: the unfiltered call's contract and protocol with every shard's local step replaced by its filtered form over the
 * shard's part.  A null shard filter, a stale or foreign one, an unknown mode / regime are errors; on any argument error nothing is written.
 *   mse_shard_group_search_filtered(_dev)  local step mse_bruteforce_topk_filtered_f16_dev(part g, id_offset = first row).  Equals
 *                                          mse_bruteforce_topk_filtered_f16 over one base of all rows with the global filter, bit for bit,
 *                                          in every mode; padding INT64_MIN / MSE_ID_NONE when fewer than k rows are allowed overall.
 *   mse_shard_group_pq_scan_topk_filtered  phase A = mse_pq_scan_topk_block_filtered(part g, r, r) per shard, phase B unchanged (every member
 *                                          of the merged top-r is allowed by construction; empty slots stay empty).  Equals
 *                                          mse_pq_scan_topk_batch_filtered over unsharded codes, bit for bit, in MSE_PQ_FILTER_SCAN, _LIST
 *                                          and _AUTO; AUTO is resolved PER SHARD by mse_pq_filtered_plan from that shard's codes and count.
 *   mse_shard_group_query_topk_filtered    every shard runs mse_disk_query_topk_block_filtered on its graph and part; the answer is the
 *                                          (score desc, id asc) merge of the per-shard mse_disk_query_topk_filtered answers.  Under
 *                                          MSE_FILTERED_AUTO EACH SHARD resolves mse_filtered_plan from its own rows and count, so shards
 *                                          of one call may run different regimes and effective search lists.
 * A shard whose part allows no row launches nothing and hands over padding. */
typedef struct mse_shard_filter mse_shard_filter;
mse_shard_filter* mse_shard_group_filter(mse_shard_group* g, const mse_filter* global);
mse_shard_filter* mse_shard_group_filter_from_local(mse_shard_group* g, const mse_filter* const* per_shard);
mse_shard_filter* mse_shard_group_live_filter(mse_shard_group* g, int and_has_url);
void mse_shard_filter_free(mse_shard_filter* sf);
size_t mse_shard_filter_count(const mse_shard_filter* sf);
size_t mse_shard_filter_n_shards(const mse_shard_filter* sf);
const mse_filter* mse_shard_filter_shard(const mse_shard_filter* sf, size_t shard);
mse_filter* mse_shard_filter_global(const mse_shard_filter* sf, int device);
int mse_shard_group_search_filtered(mse_shard_group* g, const mse_shard_filter* sf, const uint16_t* queries, size_t nq, size_t k, int mode,
                                    int64_t* scores, uint32_t* ids);
int mse_shard_group_search_filtered_dev(mse_shard_group* g, const mse_shard_filter* sf, const void* queries_dev, size_t nq, size_t k, int mode,
                                        void* scores_dev, void* ids_dev);
int mse_shard_group_pq_scan_topk_filtered(mse_shard_group* g, const mse_shard_filter* sf, const float* queries_f32, const float* scales, size_t nq,
                                          size_t r, size_t k, int mode, int64_t* scores, uint32_t* ids);
int mse_shard_group_query_topk_filtered(mse_shard_group* g, const mse_shard_filter* sf, const uint16_t* queries, const float* luts,
                                        const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k, int regime,
                                        int64_t* scores, uint32_t* ids);
/* mse_disk_query_topk_block over has_url AND allowed: the filtered request path (regimes and AUTO plan of mse_disk_query_topk_filtered) with
 * the results left on the device as a packed block, ids + id_offset; never coalesced.  The LIST regime writes the block directly. */
int mse_disk_query_topk_block_filtered(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_filter* f, int regime,
                                       const uint32_t* starts, const uint16_t* queries, const float* luts, const float* scales, size_t nq,
                                       int disable_pq, size_t beamwidth, size_t search_list, size_t k, uint64_t id_offset, void* block_dev,
                                       uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
/* One process per GPU: the filtered forms of mse_comm_search_dev / _pq_scan_topk / _query_topk.  f is THIS RANK's LOCAL filter -- the caller's
 * mse_filter_slice(global, first_row, rows of the rank, the rank's device) -- over the rank's rows; every rank must make the call. */
int mse_comm_search_filtered_dev(mse_comm* c, mse_searcher* s, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode,
                                 uint64_t id_offset, void* scores_dev, void* ids_dev);
int mse_comm_pq_scan_topk_filtered(mse_comm* c, mse_pq* pq, const mse_codes* codes, mse_searcher* s, const mse_filter* f, const float* queries_f32,
                                   const float* scales, size_t nq, size_t r, size_t k, int mode, uint64_t first_row, void* scores_dev,
                                   void* ids_dev);
int mse_comm_query_topk_filtered(mse_comm* c, mse_searcher* s, mse_pq* pq, const mse_codes* codes, const mse_graph* g, const mse_filter* f,
                                 int regime, const uint16_t* queries, const float* luts, const float* scales, size_t nq, int disable_pq,
                                 size_t beamwidth, size_t search_list, size_t k, uint64_t first_row, void* scores_dev, void* ids_dev);
/* ---- grouped search across the shards: one result per group, collapsed again where the shards' answers meet --------
 * A group's rows straddle shard boundaries, so (a) a shard needs the global grouping cut to ITS rows and relabelled to local ids, and
 * (b) the per-shard grouped answers must be collapsed once more by the GLOBAL grouping before the k best are taken.  k records per shard
 * and query are enough for (b): take the union of the shards' records in (score desc, id asc) order and keep the first record of every
 * group; a record x of group g on shard s among the first k kept is g's representative on s, and every group ranked ahead of g on s has
 * a record ahead of x in the union, so fewer than k groups precede g on s and x is in that shard's grouped top-k.  Hence
 *   collapse(merge of the per-shard grouped top-k) = collapse(merge of everything the shards ranked), cut to k,
 * and the exchange keeps its size: shards x nq x k x 12 bytes.
 *   mse_groups_slice   a fresh mse_groups over LOCAL rows [0, n_rows) that induces the partition src induces on rows [first_row, first_row
 *                      + n_rows).  Labels are canonical: a grouped row's local label is the local id of the FIRST row of its group inside
 *                      the slice; MSE_GROUP_NONE stays.  Rows at or past mse_groups_len(src) are groups of their own: the result is as
 *                      long as the part of the slice inside src, and a slice wholly past src is the empty grouping (length 0, count 0),
 *                      under which every row is a group of its own.  count as mse_groups_count defines it.  device: where the result
 *                      lives, -1 = src's device; for another device the labels of the slice go over by ONE peer copy and are relabelled
 *                      there.  Transient scratch: 4 bytes x mse_groups_len(src) on the result's device, freed before return.  n_rows =
 *                      0, a null grouping and a device ordinal out of range are errors.  Deterministic (an atomic min of the local id
 *                      per label, then a lookup).
 *   mse_groups_read    the label array, mse_groups_len(g) u32, to the host.
 * mse_shard_groups: the grouping of a shard group's GLOBAL rows, cut for its shards -- what the grouped searches of the group take.
 *   mse_shard_group_groups   mse_groups_slice of `global` at each shard's first row and length, on the shard's device, plus a copy of the
 *                            global label array on the root device (the device of shard 0), which the merge looks up by global row id.
 *                            A grouping shorter than the group leaves the rows past it groups of their own; one longer than max(first
 *                            row + rows) over the shards is an error.
 *   mse_shard_groups_part    shard g's local grouping, BORROWED (it lives as long as the object); NULL without an error for a shard that
 *                            lies wholly past the grouping -- such a shard runs its ungrouped call, which by contract answers the same --
 *                            and NULL with the error set for a shard index out of range.
 *   mse_shard_groups_n_shards its parts
 * It carries the group's layout stamp exactly as mse_shard_filter does: one made for another group, or from before a re-fill
 * (mse_shard_group_generate, _load_host, _set_shard_device), is refused by every call that takes one.  It is immutable, holds no reference
 * to the group or to `global`, and must outlive the calls it is passed to.
 * The grouped merge: one workgroup per query over the gathered packed blocks IN PLACE -- of every group (group_of[global id]; a record of
 * group MSE_GROUP_NONE or with an id at or past the grouping is a group of its own) the best record by (score desc, id asc) stays, every
 * other record of the group becomes the hole (INT64_MIN, MSE_ID_NONE); holes and padding already in the blocks are skipped; the
 * unchanged selection of mse_merge_topk_packed_dev then takes the k best.  Integer atomics only: bit-reproducible.  The table lives in
 * LDS up to n_shards x k_in = 4096 records per query and in global memory (scratch of the searcher) beyond, up to 8 x 1984 and more.
 *   mse_merge_topk_packed_grouped_dev  mse_merge_topk_packed_dev with that step first; k_in records per shard and query in the blocks
 *                                      (0: k_in = k), the k best representatives out.  groups_global must live on the searcher's
 *                                      device.  The blocks are CHANGED in place (non-representatives become holes).  Asynchronous on
 *                                      the searcher's stream.  What a process-per-GPU caller runs after its own all-gather.
 * The three searches take sg (non-null) and an optional shard filter sf.  Lock discipline and validation order of the _filtered sibling
 * (whose checks apply only when sf is given); then "null shard groups", an error of its own; then the fit of sg.
 *   mse_shard_group_search_grouped(_dev)   local step mse_bruteforce_topk_grouped_f16_dev(part g, filter part or NULL, id_offset = first
 *                                          row), exchange, grouped merge.  Equals mse_bruteforce_topk_grouped_f16 over one base of all
 *                                          rows with the global grouping (and filter), bit for bit, in every mode.
 *   mse_shard_group_query_topk_grouped     every shard runs mse_disk_query_topk_block_grouped on its graph and part (regime as in the
 *                                          filtered call when sf is given), then the grouped merge: the collapse of the merge of what
 *                                          the shards visited.  An approximate search; a short answer shows as padding, as on one GPU.
 *   mse_shard_group_pq_scan_topk_grouped   phases A and B of mse_shard_group_pq_scan_topk (A filtered when sf is given); phase B's final
 *                                          merge is the grouped merge: the collapse of the exactly re-ranked global top-r, k of it,
 *                                          padded when the r candidates hold fewer than k groups.
 * mse_shard_group_last_timing keeps its meaning; [2] includes the group step.
 * Not covered: mse_comm_*_grouped (every rank would need the global labels; mse_merge_topk_packed_grouped_dev is the building block),
 * an unsharded grouped PQ scan, groupings over mutated graphs after mse_graph_compact (by row id, as on one GPU), bench.py. */
mse_groups* mse_groups_slice(const mse_groups* src, uint64_t first_row, size_t n_rows, int device);
int mse_groups_read(const mse_groups* g, uint32_t* out);
typedef struct mse_shard_groups mse_shard_groups;
mse_shard_groups* mse_shard_group_groups(mse_shard_group* g, const mse_groups* global);
const mse_groups* mse_shard_groups_part(const mse_shard_groups* sg, size_t shard);
size_t mse_shard_groups_n_shards(const mse_shard_groups* sg);
void mse_shard_groups_free(mse_shard_groups* sg);
int mse_merge_topk_packed_grouped_dev(mse_searcher* s, const mse_groups* groups_global, void* gathered_blocks_dev, size_t n_shards, size_t nq,
                                      size_t k_in, size_t k, void* out_scores_dev, void* out_ids_dev);
int mse_shard_group_search_grouped(mse_shard_group* g, const mse_shard_groups* sg, const mse_shard_filter* sf, const uint16_t* queries, size_t nq,
                                   size_t k, int mode, int64_t* scores, uint32_t* ids);
int mse_shard_group_search_grouped_dev(mse_shard_group* g, const mse_shard_groups* sg, const mse_shard_filter* sf, const void* queries_dev,
                                       size_t nq, size_t k, int mode, void* scores_dev, void* ids_dev);
int mse_shard_group_pq_scan_topk_grouped(mse_shard_group* g, const mse_shard_groups* sg, const mse_shard_filter* sf, const float* queries_f32,
                                         const float* scales, size_t nq, size_t r, size_t k, int mode, int64_t* scores, uint32_t* ids);
int mse_shard_group_query_topk_grouped(mse_shard_group* g, const mse_shard_groups* sg, const mse_shard_filter* sf, const uint16_t* queries,
                                       const float* luts, const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list,
                                       size_t k, int regime, int64_t* scores, uint32_t* ids);
/* mse_disk_query_topk_block with one result per group of `groups` (non-null; LOCAL row ids) over has_url AND f (f may be NULL: the
 * unfiltered traversal, regime ignored): the grouped request path (mse_disk_query_topk_grouped) with the results left on the device as a
 * packed block, ids + id_offset; never coalesced. */
int mse_disk_query_topk_block_grouped(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const mse_groups* groups,
                                      const mse_filter* f, int regime, const uint32_t* starts, const uint16_t* queries, const float* luts,
                                      const float* scales, size_t nq, int disable_pq, size_t beamwidth, size_t search_list, size_t k,
                                      uint64_t id_offset, void* block_dev, uint32_t* n_visited, uint32_t* cmps, uint32_t* pq_cmps);
/* measurement hook of the row-gather kernel of mse_graph_compact (for scripts/graph_compact_probe.py): *last_gather_ms (or null)
 * receives the HIP-event time of that kernel in the last mse_graph_compact made on s while the switch was on (0: none), then the
 * switch is set (0 off, 1 on, 2 on and reset).  The kernel reads n_live and writes capacity rows of 2 d + code_size + n_desc bytes. */
int mse_searcher_compact_timing(mse_searcher* s, int enable, double* last_gather_ms);
/* D2H, for spot checks, like mse_base_read_rows: codes_out [n][code_size], desc_out_or_null [n][n_desc] */
int mse_codes_read_rows(const mse_codes* c, size_t first, size_t n, uint8_t* codes_out, uint8_t* desc_out_or_null);
/* test hook: the base's cached norm bound as float bits -- [0] largest row norm x 1.0001, [1] largest subnormal mass of a row
 * x 1.0001, [2] largest |component| -- measured first if it is not ready */
int mse_debug_base_norm_bits(const mse_base* b, uint32_t out[3]);
/* diskann::greedy_search (lib.rs:183-211) GPU-resident and batched over queries (the in-RAM scorer, A21): one
 * workgroup per query, outputs as mse_greedy_search leaves them in `buf`: buf_ids/buf_scores [nq][search_list]
 * (first buf_len[q] valid, best first), n_distances [nq] = GreedySearchCounters.distances. */
int mse_graph_search_batch(mse_searcher* s, const mse_graph* g, const uint32_t* starts, const uint16_t* queries, size_t nq,
                           size_t search_list, int base_vectors_only, uint32_t query_breakpoint, uint32_t* buf_ids,
                           int64_t* buf_scores, uint32_t* buf_len, uint32_t* n_distances);

/* The same with the caller's two preparation steps (src/query_disk_index.rs:475-477) done on the device: queries arrive
 * as f32 [nq][d]; their f16 copies (RNE, half::f16::from_f32) score the fetched nodes and preprocess_query
 * (vector.rs:367-384) makes the distance tables in HBM, so 64 KiB per query stay off PCIe. */
int mse_disk_search_batch_f32(mse_searcher* s, mse_pq* pq, const mse_codes* c, const mse_graph* g, const uint32_t* starts,
                              const float* queries_f32, const float* scales, size_t nq, int disable_pq, size_t beamwidth,
                              size_t search_list, uint32_t* buf_ids, int64_t* buf_scores, uint32_t* buf_len,
                              uint32_t* visited_ids, int64_t* visited_scores, size_t visited_cap, uint32_t* n_visited,
                              uint32_t* cmps, uint32_t* pq_cmps);
/* Result de-duplication of the visited list (src/query_disk_index.rs:482-527): S = V V^T over the visited rows
 * (ids into the searcher's base, visit order), greedy keep-first filter with S[i][j] > threshold (0.95, :99) against
 * already kept rows.  keep[i] = 1 for survivors. */
int mse_dedup_visited(mse_searcher* s, const uint32_t* ids, size_t n, float threshold, uint8_t* keep);
/* Shard / entry-point selection (src/query_disk_index.rs:254-256,447-450): argmax over shard centroids of
 * scale_dot_result_f64(dot_f32(centroid, query)), LAST maximum on ties (position_max_by_key). */
int mse_select_shard(const float* centroids, size_t n_shards, size_t d, const float* query, size_t* shard_out);
/* medioid (diskann/src/lib.rs:52-68): row with the largest `dot` (vector.rs:49-52) against the f16-rounded running
 * mean of all rows; last maximum on ties. */
int mse_medioid(const mse_base* b, uint32_t* id_out);

/* ---- Index packing (dump_processor; quantize_batch is mse_pq_quantize_batch above) ----
 * ScoreModel::score_batch (src/score_model.rs:13-32): out[b] = down_proj . silu(up_proj . x_b + bias) * d_emb / d_hidden.
 * up_proj [d_hidden][d_emb], bias [d_hidden], down_proj [out_channels][d_hidden], row-major f32 (the safetensors layout). */
typedef struct mse_score_model mse_score_model;
mse_score_model* mse_score_model_load(const float* up_proj, const float* bias, const float* down_proj, size_t d_emb,
                                      size_t d_hidden, size_t out_channels);
void mse_score_model_free(mse_score_model* m);
size_t mse_score_model_output_channels(const mse_score_model* m);
int mse_score_model_score_batch(mse_score_model* m, const float* input, size_t batch, float* out /* [batch][out_channels] */);
/* Descriptor bytes (src/dump_processor.rs:483-491): out[i][j] = position of scores[i][j] in the ascending cdfs[j]
 * as `binary_search_by(|x| x.partial_cmp(score))` reports it (Ok(p) or Err(p) -> p), one byte; cdf_len <= 255
 * (meme-rater/compute_cdf.py: 255 quantiles, 255 = above the last). */
int mse_descriptor_buckets(const float* cdfs, size_t n_desc, size_t cdf_len, const float* scores, size_t n, uint8_t* out);

/* ---- Descriptors of a resident index: scores, CDFs and descriptor bytes without the rows or the activations crossing PCIe ----
 * mse_scores: a device-resident score table, [n][channels] f32 plus an optional u32 timestamp channel (channel index `channels`).
 *   mse_scores_from_base   ScoreModel::score_batch (src/score_model.rs:13-32) over decode_fp16_buffer of the base's rows (the widening is
 *                          exact), fused on the f32 matrix cores: rows ids[i], i < n (any order, repeats allowed; each < mse_base_len), or
 *                          first .. first + n when ids is NULL.  The model's d_emb must equal the base's d and it has at most 8 output
 *                          channels.  The summation orders are fixed (csrc/describe.hip) and name neither the row's place in the call nor
 *                          the call's size: a row's score bits are the same however it is asked for.  timestamps: host [n] or NULL, each in
 *                          [0, 2^32) (the extra channel of meme-rater/compute_cdf.py:61-62).
 *   mse_scores_from_f16    the same kernel over f16 rows the caller holds on the host, [n_rows][d] of ANY width d >= 1 (a base's is a
 *                          multiple of 64), uploaded for the call to the current device: rows that are in no base yet.
 *   mse_scores_from_host   the same table from scores the caller has already (on the current device).
 * Errors leave the model, the base and the codes as they were. */
typedef struct mse_scores mse_scores;
mse_scores* mse_scores_from_base(mse_score_model* m, const mse_base* b, const uint32_t* ids_or_null, size_t first, size_t n,
                                 const int64_t* timestamps_or_null);
mse_scores* mse_scores_from_f16(mse_score_model* m, const uint16_t* rows_f16, size_t n_rows, size_t d, const uint32_t* ids_or_null, size_t first,
                                size_t n, const int64_t* timestamps_or_null);
mse_scores* mse_scores_from_host(const float* scores, size_t n, size_t n_channels, const int64_t* timestamps_or_null);
void mse_scores_free(mse_scores* s);
size_t mse_scores_len(const mse_scores* s);
size_t mse_scores_channels(const mse_scores* s);       /* the f32 channels; the timestamps are one more */
int mse_scores_has_timestamps(const mse_scores* s);
int mse_scores_read(const mse_scores* s, float* out /* [n][channels] */, uint32_t* ts_out_or_null /* [n] */);
/* out[i] = the value at rank ranks[i] (0-based, < n) of the channel's ascending order -- numpy.sort(x)[ranks], which is what
 * numpy.quantile partitions for (meme-rater/compute_cdf.py:69) -- exactly, without sorting: a three-pass radix select (11 / 11 / 10 bits)
 * over keys that order f32 with -0.0 == +0.0 (the timestamps: plain u32), in scratch of fixed size, integer atomics only.  Any number of
 * ranks (512 per select).  A NaN among the keys fails the call with their count (the reference's partial_cmp().unwrap() panics,
 * src/dump_processor.rs:483-491); +-inf are ordinary keys.  n < 2^32. */
int mse_scores_order_statistics(const mse_scores* s, size_t channel, const uint64_t* ranks, size_t n_ranks, double* out);
/* cdfs_out [channels (+ 1 with timestamps)][cdf_len] = numpy.quantile(channel, numpy.linspace(0, 1, cdf_len)) narrowed to f32
 * (meme-rater/compute_cdf.py:64-71; IndexHeader.descriptor_cdfs): order statistics from the device, numpy's interpolation in float64
 * on the host.  1 <= cdf_len <= 255. */
int mse_scores_fit_cdfs(const mse_scores* s, size_t cdf_len, float* cdfs_out);
/* desc[row][j] = mse_descriptor_buckets' byte of value_j in cdfs[j] for row = ids[i] (distinct; or first + i), i < mse_scores_len(s):
 * value_j = scores[i][j], and (float)timestamp[i] for the last channel (src/dump_processor.rs:481-491), written in place into the codes'
 * descriptor bytes; other rows keep theirs.  The codes must carry channels (+ 1 with timestamps) descriptor bytes per row.  With a
 * graph, the write happens under the graph's exclusive lock, as mse_graph_insert_rows does. */
int mse_codes_describe(mse_codes* c, mse_graph* graph_or_null, const mse_scores* s, const uint32_t* ids_or_null, size_t first, const float* cdfs,
                       size_t cdf_len);
/* measurement hook (scripts/describe_probe.py): HIP-event milliseconds of the score kernel of the last mse_scores_from_base and of the
 * three counting passes of the last select made while the switch was on; then the switch is set (0 off, 1 on, 2 on and reset). */
int mse_describe_timing(int enable, double* mlp_ms_or_null, double* select_pass_ms_or_null /* [3] */);

/* ---- Sparse-autoencoder features of a resident index (the reference's sae/): the encode on the device, without the rows leaving it ----
 * SAE.forward up to the mask (sae/model.py:31-41): a = relu(up_proj(x)), t = kthvalue(a, d_hidden - top_k) -- the (top_k + 1)-th largest --
 * and the kept set { j : a_j > t }, strictly: at most top_k features, fewer where values tie at t (model.py:37-40).  The checkpoint's
 * tensors as torch stores them: up [d_hidden][d_emb] (up_proj.weight), up_bias [d_hidden] or NULL (up_proj_bias = False at
 * sae/train.py:25-33, where d_hidden = 262144 and top_k = 128), down [d_emb][d_hidden] (down_proj.weight), down_bias [d_emb] or NULL;
 * all f32, host pointers, copied (down is kept transposed).  1 <= top_k <= 256, top_k < d_hidden, d_emb >= 1.
 * The arithmetic is fixed (csrc/sae.hip states it, tests/sae_ref.py restates it): the pre-activation is one k-ascending f32 fma chain
 * from +0 (the f32 matrix cores), the bias one f32 add; a row's features come in canonical order -- activation descending, feature
 * ascending -- and do not depend on the row's place in the call, the call's size, ids versus range or how d_hidden is split.  (The
 * reference runs these products in TF32, sae/shared.py:4, and so pins no bits.)  A row with a NaN pre-activation is invalid: its count
 * reads 0xFFFFFFFF, it holds no features and counts nowhere; +inf is an ordinary value. */
typedef struct mse_sae mse_sae;
typedef struct mse_features mse_features;
mse_sae* mse_sae_load(const float* up, const float* up_bias_or_null, const float* down, const float* down_bias_or_null, size_t d_emb,
                      size_t d_hidden, size_t top_k);
void mse_sae_free(mse_sae* m);
size_t mse_sae_d_emb(const mse_sae* m);
size_t mse_sae_d_hidden(const mse_sae* m);
size_t mse_sae_top_k(const mse_sae* m);
/* The feature table of rows ids[i], i < n (any order, repeats allowed; each < mse_base_len), or first .. first + n when ids is NULL.
 * count_features != 0: every kept feature of every valid row adds one to the model's counters (feature_activation_counter,
 * model.py:23,42).  The table borrows the base's rows (mse_features_reconstruct reads them): the caller keeps the base alive.
 * mse_sae_encode_f16: the same over f16 rows on the host, [n_rows][d] of any width d >= 1, of which the table keeps a device copy.
 * Errors (a width that is not the model's, an id past the base, a wrapped base over host memory) leave the model and the base usable. */
mse_features* mse_sae_encode_base(mse_sae* m, const mse_base* b, const uint32_t* ids_or_null, size_t first, size_t n, int count_features);
mse_features* mse_sae_encode_f16(mse_sae* m, const uint16_t* rows_f16, size_t n_rows, size_t d, int count_features);
void mse_features_free(mse_features* f);
size_t mse_features_len(const mse_features* f);
size_t mse_features_top_k(const mse_features* f);
uint64_t mse_features_invalid_rows(const mse_features* f);
/* counts [n] (0xFFFFFFFF: invalid row), features [n][top_k] (unused slots 0xFFFFFFFF), activations [n][top_k] (unused slots +0); any
 * of the three may be NULL */
int mse_features_read(const mse_features* f, uint32_t* counts_or_null, uint32_t* features_or_null, float* activations_or_null);
/* down_proj over the kept features (model.py:43) and the row's share of mse_loss (sae/train.py:55-56): recon [n][d_emb] with
 * r_d = fma(a, down[d][f], r_d) over the row's features in canonical order from down_bias[d] (or +0); sqerr [n] = sum over d of
 * (f32(r_d - x_d))^2 in f64, in the fixed order csrc/sae.hip states.  An invalid row gives NaN in both.  m must be the model that made
 * the table. */
int mse_features_reconstruct(const mse_features* f, mse_sae* m, float* recon_or_null, double* sqerr_or_null);
/* The rows that keep `feature` with an activation >= min_activation, as a filter over n_rows base rows (row ids[i], or first + i; a
 * table made from host rows: i), built on the device (mse_filter_from_bits_dev) and usable wherever a filter is.  n_rows must cover
 * every row the table speaks of. */
mse_filter* mse_features_filter(const mse_features* f, uint32_t feature, float min_activation, size_t n_rows);
/* out [d_hidden] = the counters; reset != 0 zeroes them after the read (reset_counters, model.py:26-29, returns the old values) */
int mse_sae_counters(mse_sae* m, uint64_t* out_or_null, int reset);
/* test and probe hook: split d_hidden over `parts` workgroups per row tile (1 .. 1024; fewer when there are fewer hidden tiles);
 * 0 = automatic, enough parts for two workgroups per CU.  The answer does not depend on it. */
int mse_sae_set_hidden_parts(mse_sae* m, int parts);
/* measurement hook (scripts/sae_probe.py): HIP-event milliseconds of the encode and of the merge launches of the last encode made
 * while the switch was on; then the switch is set (0 off, 1 on, 2 on and reset). */
int mse_sae_timing(int enable, double* encode_ms_or_null, double* merge_ms_or_null);
/* The model's current weights (a trainer changes them): up [d_hidden][d_emb], up_bias [d_hidden], down [d_emb][d_hidden] as the
 * checkpoint stores it, down_bias [d_emb]; any may be NULL, and a bias the model was loaded without is left unwritten. */
int mse_sae_read_weights(mse_sae* m, float* up_or_null, float* up_bias_or_null, float* down_or_null, float* down_bias_or_null);

/* ---- Sparse-autoencoder training over a resident index (the reference's sae/train.py:51-59): mse_loss, backward and
 * torch.optim.AdamW on the device, over an mse_sae whose device weights are updated in place.  The forward pass is the encode above;
 * the arithmetic of the backward pass and of the update is fixed (csrc/sae_train.hip states it, tests/sae_train_ref.py restates it),
 * so a run is the same bytes however it is cut into calls, from ids or from host rows, and run to run.  The model needs a down_bias
 * (the reference's decoder always has one).  The trainer must be freed before its model; a trainer whose model was freed refuses every
 * call.  beta1, beta2 and eps act in f32; lr, weight_decay and the bias corrections are combined in double. */
typedef struct mse_sae_trainer mse_sae_trainer;
mse_sae_trainer* mse_sae_trainer_create(mse_sae* m, double lr, double beta1, double beta2, double eps, double weight_decay);
void mse_sae_trainer_free(mse_sae_trainer* tr);
/* completed steps (torch's `step`) */
uint64_t mse_sae_trainer_step_count(const mse_sae_trainer* tr);
/* n_steps steps of `batch` rows each: step s trains on rows ids[s * batch + i], i < batch, of the base (any order, repeats allowed).
 * batch * top_k <= 65536.  A step with an invalid (NaN) row or a non-finite loss is refused: weights, moments, step count and feature
 * counters stay as they were and the later steps of the call are not run; *steps_done_out tells how many steps completed (the call
 * still returns 0) and losses_out [n_steps] holds that many losses (F.mse_loss of each step, before its update).  The call holds the
 * model's lock and gives the model a new serial: an mse_features made before it is refused by mse_features_reconstruct.  Errors (a
 * width that is not the model's, batch * top_k over the limit, an id past the base) leave every handle usable.
 * mse_sae_trainer_steps_f16: the same over n_steps * batch f16 rows on the host, [.][d]. */
int mse_sae_trainer_steps(mse_sae_trainer* tr, const mse_base* b, const uint32_t* ids, size_t batch, size_t n_steps, double* losses_out,
                          size_t* steps_done_out);
int mse_sae_trainer_steps_f16(mse_sae_trainer* tr, const uint16_t* rows_f16, size_t d, size_t batch, size_t n_steps, double* losses_out,
                              size_t* steps_done_out);
/* The optimizer's state: the step count and exp_avg / exp_avg_sq of every parameter in the checkpoint's layout (up's [d_hidden][d_emb],
 * down's [d_emb][d_hidden]); the encoder bias's only where the model has one.  Read: any pointer may be NULL.  Write: all are needed. */
int mse_sae_trainer_state_read(mse_sae_trainer* tr, uint64_t* t_out, float* m_up, float* v_up, float* m_up_bias_or_null, float* v_up_bias_or_null,
                               float* m_down, float* v_down, float* m_down_bias, float* v_down_bias);
int mse_sae_trainer_state_write(mse_sae_trainer* tr, uint64_t t, const float* m_up, const float* v_up, const float* m_up_bias_or_null,
                                const float* v_up_bias_or_null, const float* m_down, const float* v_down, const float* m_down_bias,
                                const float* v_down_bias);
/* test and probe hook: with weight_decay = 0 the dense update leaves out feature rows that have never had a member (they do not move);
 * 0 turns that off.  The bytes do not depend on it. */
int mse_sae_trainer_set_skip(mse_sae_trainer* tr, int enable);
/* measurement hook (scripts/sae_train_probe.py): out [4] = HIP-event milliseconds of the forward passes (with the gate), of the small
 * backward kernels and of the dense update of the last training call made while the switch was on, and the steps they cover; then the
 * switch is set (0 off, 1 on, 2 on and reset). */
int mse_sae_trainer_timing(int enable, double* out_or_null /* [4] */);

/* ---- The ensemble rater of the reference's meme-rater/ on the device: the quality model whose scores become descriptor bytes, trained
 * from rated pairs of resident rows, scored member by member, asked where its members disagree, exported as the wide score model.
 * meme-rater/model.py:18-52: n_members one-hidden-layer MLPs (Linear d_emb -> d_emb, silu, Linear d_emb -> out_channels) under a
 * Bradley-Terry head, p = sigmoid(score(first) - score(second)).  The weights live in the wide layout of
 * ensemble_to_wide_model.py:44-55, all f32: up [n_members * d_emb][d_emb], bias [n_members * d_emb], down [out_channels][n_members *
 * d_emb]; member m owns hidden units m * d_emb .. (m + 1) * d_emb.  The output layer's bias is not carried: the win probability is
 * shift-invariant, its gradient is g - g = 0, and the export zeroes it (ensemble_to_wide_model.py:36-37).  One hidden layer only (the
 * export's own TODO at :43), no dropout (train.py:40 trains with 0.0).  1 <= n_members <= 64, 1 <= out_channels <= 8.
 * The arithmetic is fixed (csrc/rater.hip states it, tests/rater_ref.py restates it, bit for bit): the exponential is
 * csrc/rater_math.h's, written in correctly rounded f32 operations only. */
typedef struct mse_rater mse_rater;
typedef struct mse_rater_trainer mse_rater_trainer;
typedef struct mse_member_scores mse_member_scores;
/* host pointers, copied */
mse_rater* mse_rater_create(const float* up, const float* bias, const float* down, size_t d_emb, size_t n_members, size_t out_channels);
void mse_rater_free(mse_rater* r);
/* the current device weights (a trainer changes them), the arguments of mse_rater_create; any may be NULL */
int mse_rater_read_weights(mse_rater* r, float* up_or_null, float* bias_or_null, float* down_or_null);
/* meme-rater/train.py:61: torch.optim.AdamW over every parameter, in place on the rater's device weights.  beta1, beta2 and eps act
 * in f32; lr, weight_decay and the bias corrections are combined in double.  The trainer must be freed before its
 * rater; a trainer whose rater was freed refuses every call. */
mse_rater_trainer* mse_rater_trainer_create(mse_rater* r, double lr, double beta1, double beta2, double eps, double weight_decay);
void mse_rater_trainer_free(mse_rater_trainer* tr);
/* completed steps (torch's `step`) */
uint64_t mse_rater_trainer_step_count(const mse_rater_trainer* tr);
/* n_steps steps of train_step (train.py:63-71: F.binary_cross_entropy on the win probabilities, backward, optimizer.step) with `batch`
 * pairs per member, 1 <= batch <= 64: in step s member m sees the pairs pair_ids[s][m][b][0 .. 2] -- rows of the base, first and
 * second; each member its own data order as train.py:116-118 gives it -- with targets[s][m][b][c] in [0, 1].  The ids are checked
 * against the base and uploaded once; the steps are queued without a host round trip.  A step with a non-finite row or a non-finite
 * loss is refused: weights, moments and step count stay as they were and the later steps of the call are not run; *steps_done_out tells
 * how many steps completed (the call still returns 0) and losses_out [n_steps] holds that many losses (each step's, before its update).
 * Errors (a width that is not the rater's, a batch over the limit, an id past the base) leave every handle usable.
 * mse_rater_trainer_steps_f16: the same over f16 rows on the host, [n_rows][d], uploaded once, and indices into them. */
int mse_rater_trainer_steps(mse_rater_trainer* tr, const mse_base* b, const uint32_t* pair_ids /* [n_steps][M][batch][2] */,
                            const float* targets /* [n_steps][M][batch][C] */, size_t batch, size_t n_steps, double* losses_out,
                            size_t* steps_done_out);
int mse_rater_trainer_steps_f16(mse_rater_trainer* tr, const uint16_t* rows_f16, size_t n_rows, size_t d, const uint32_t* pair_idx,
                                const float* targets, size_t batch, size_t n_steps, double* losses_out, size_t* steps_done_out);
/* The optimizer's state, what save_ckpt keeps beside the weights (train.py:98-102): the step count and exp_avg / exp_avg_sq of up,
 * bias and down in the wide layout.  Read: any pointer may be NULL.  Write: all are needed. */
int mse_rater_trainer_state_read(mse_rater_trainer* tr, uint64_t* t_out, float* m_up, float* v_up, float* m_bias, float* v_bias, float* m_down,
                                 float* v_down);
int mse_rater_trainer_state_write(mse_rater_trainer* tr, uint64_t t, const float* m_up, const float* v_up, const float* m_bias, const float* v_bias,
                                  const float* m_down, const float* v_down);
/* test hook: the scores s [M][2 * batch][C] the forward pass of the last completed step of the last call made of its slots (slot 2 b is
 * pair b's first row); *batch_out = that step's batch.  An error where the last call ended in a refusal or no call was made. */
int mse_rater_trainer_last_scores(mse_rater_trainer* tr, float* out_or_null, size_t* batch_out_or_null);
/* measurement hook (scripts/rater_probe.py): out [4] = HIP-event milliseconds of the forward passes, of the small backward kernels and
 * of the dense update of the last training call made while the switch was on, and the steps they cover; then the switch is set (0 off,
 * 1 on, 2 on and reset). */
int mse_rater_trainer_timing(int enable, double* out_or_null /* [4] */);
/* Every member's scores of rows ids[i], i < n (any order, repeats allowed; each < mse_base_len), or first .. first + n when ids is
 * NULL: a device table [n][M][C] of the rule's s, unscaled (model.py:38, the ensemble's stacked outputs without the output bias).  A
 * row's scores are the same bits however it is asked for, and the bits the trainer's forward pass makes of that row.
 * mse_member_scores_from_f16: the same over f16 rows on the host, [n_rows][d]. */
mse_member_scores* mse_member_scores_from_base(mse_rater* r, const mse_base* b, const uint32_t* ids_or_null, size_t first, size_t n);
mse_member_scores* mse_member_scores_from_f16(mse_rater* r, const uint16_t* rows_f16, size_t n_rows, size_t d, const uint32_t* ids_or_null,
                                              size_t first, size_t n);
void mse_member_scores_free(mse_member_scores* s);
size_t mse_member_scores_len(const mse_member_scores* s);
int mse_member_scores_read(const mse_member_scores* s, float* out /* [n][M][C] */);
/* active_learning.py:50-53: out[i] = max over channels of torch.var over members (correction 1) of the win probabilities
 * sigmoid(s[a_idx[i]] - s[b_idx[i]]), indices into the table; in the fixed order csrc/rater.hip states.  A table of one member is
 * refused. */
int mse_member_scores_pair_variance(mse_member_scores* s, const uint32_t* a_idx, const uint32_t* b_idx, size_t n_pairs, float* out /* [n_pairs] */);

/* ---- SigLIP ViT image tower: the in-process seam of clip_server.py, `fast_image_fns[batch](images NCHW
 * fp16 on device) -> [batch, 1152]` (clip_server.py:31,66-82,105-112), plus the normalisation and fp16
 * serialisation of do_inference / run_inference (clip_server.py:115,166).  Graph: aitemplate/model.py:13-123;
 * hyper-parameters aitemplate/run.py:47-55; weight names clip_server.py:40-57 without the "visual." prefix. */
typedef struct mse_siglip mse_siglip;
typedef struct mse_siglip_config {
    int img_size;    /* 384 */
    int patch_size;  /* 14 */
    int in_chans;    /* 3 */
    int emb_dim;     /* 1152 */
    int depth;       /* 27 */
    int num_heads;   /* 16 */
    int mlp_dim;     /* 4304 */
    float eps;       /* LayerNorm epsilon, 1e-6 */
    int gelu_tanh;   /* 0 = erf GELU (timm / AITemplate "gelu"), 1 = tanh approximation (HF / big_vision) */
    int max_batch;   /* `max_batch_size` of clip_server_config.json */
} mse_siglip_config;
mse_siglip* mse_siglip_create(const mse_siglip_config* cfg);
void mse_siglip_destroy(mse_siglip* m);
int mse_siglip_n_weights(const mse_siglip* m);
const char* mse_siglip_weight_name(const mse_siglip* m, int idx);   /* names the engine expects, sorted */
/* fp32 host tensor in its state-dict shape (e.g. qkv.weight [3456,1152], patch_embed.proj.weight [1152,3,14,14]) */
int mse_siglip_set_weight(mse_siglip* m, const char* name, const float* data, const size_t* shape, int ndim);
int mse_siglip_finalize(mse_siglip* m);                              /* fails if a weight is missing */
/* images: [batch,3,H,W], dtype 0 = f32 / 1 = f16, already normalised (x/127.5 - 1); batch > max_batch is an
 * error (the reference asserts, clip_server.py:139).  Outputs (either may be NULL) are host [batch, emb_dim].
 * Batch invariance: rows of calls of >= 5 images are bit-equal whatever the batch and however many streams
 * (MSE_SIGLIP_STREAMS) the call is split over -- every kernel is chosen from the call, never from the size of one of its
 * sub-batches.  Calls of 1-4 images run small-batch kernels with another summation order: an image embedded alone (query
 * time) and the same image inside a larger batch (index time) agree to bf16 rounding (cosine within 1e-4; both within 1e-3 of
 * the fp32 model), not bit for bit.  A pipeline that needs index/query bit-equality sets MSE_SIGLIP_NOSMALL=1 in the
 * environment before mse_siglip_create (read once, there): calls of every size, one image included, then return the rows of
 * a larger batch bit for bit -- as long as no attention row raises its running maximum after its first 32 keys (true of Gaussian-regime
 * weights; with sharper logits calls of 1-2 images differ from larger batches in the last bits: DESIGN.md 3.4, "Open"). */
int mse_siglip_encode_image(mse_siglip* m, const void* images, int dtype, int on_device, int batch, int normalize,
                            float* out_f32, uint16_t* out_f16);
/* Same from decoded RGB bytes [batch][H][W][3] (host): the ToTensor / Normalize(0.5, 0.5) / .half() / stack steps of the
 * preprocessing thread (clip_server.py:131-146) run on the device; x / 127.5 - 1 in fp32, fp16 round-to-nearest-even. */
int mse_siglip_encode_rgb8(mse_siglip* m, const uint8_t* rgb_hwc, int batch, int normalize, float* out_f32, uint16_t* out_f16);
/* Same from the request bytes themselves when they are what the reference's clients send (src/common.rs:31-54: 24-bit
 * uncompressed BMP of exactly image_size): the host reads the 54-byte header, the device does BGR -> RGB, the bottom-up row
 * flip and the normalisation.  Any other file (or size) is an error: decode it on the host and use mse_siglip_encode_rgb8.
 * mse_bmp24_info is the header check alone (0 = plain 24-bit BMP; width / height / pixel_offset / bottom_up may be NULL). */
int mse_bmp24_info(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height, uint32_t* pixel_offset, int* bottom_up);
int mse_siglip_encode_bmp(mse_siglip* m, const uint8_t* const* bmps, const size_t* sizes, int batch, int normalize, float* out_f32,
                          uint16_t* out_f16);
/* ---- Resize on the device: `resize_for_embed_sync` (src/common.rs:31-54), the step every image takes before it is embedded.  The
 * image is squashed to exactly the target size with a two-pass convolution resize -- Hamming window when BOTH sides shrink, Lanczos3
 * otherwise (common.rs:44), one filter for both passes, horizontal pass first into a u8 intermediate, a pass whose input and output
 * lengths agree skipped, an image already of the target size copied.  The arithmetic is Pillow's 8-bit resample (weights in double on
 * the host, integer coefficients of 22 fractional bits, int32 sums: tests/resize_ref.py restates it), bit for bit; the reference links
 * the fast_image_resize crate, whose coefficient precision may differ in the last bit of a pixel.
 * Limits, checked before anything is launched: widths and heights 1 .. 16384, no NULL pointer, a known filter, batch >= 1 (and
 * <= max_batch for the engine calls).  Device staging is bounded: a call is processed in sub-batches of at most 1024 images whose
 * uploads, intermediates, coefficient tables (and u8 results, for mse_resize_rgb8) stay below 256 MiB together, except that one image
 * always goes through alone whatever it takes (16384 x 16384 -> 384 x 384: 786 MiB).  The tables of a sub-batch exist once more in
 * host memory while they go up. */
#define MSE_RESIZE_AUTO 0      /* the reference's rule (common.rs:44) */
#define MSE_RESIZE_HAMMING 1
#define MSE_RESIZE_LANCZOS3 2
/* Host only (no device): the coefficient table of one axis, `in` -> `out` samples, filter MSE_RESIZE_HAMMING or _LANCZOS3 (src/common.rs:31-54).
 * *ksize = row length of the table; bounds_out [out][2] = (first input sample, taps) of every output; coefs_out [out][ksize] = the
 * integer weights, zero past the taps.  bounds_out / coefs_out may be NULL: size query. */
int mse_resize_coeffs(int in, int out, int filter, int* ksize, int32_t* bounds_out, int32_t* coefs_out);
/* Host only: the filter a w x h image resized to out_w x out_h gets (src/common.rs:31-54, the rule at :44): `filter` itself unless it is
 * MSE_RESIZE_AUTO, then MSE_RESIZE_HAMMING when w > out_w and h > out_h, else MSE_RESIZE_LANCZOS3.  -1 for a refused argument. */
int mse_resize_pick_filter(int w, int h, int out_w, int out_h, int filter);
/* Resize alone (src/common.rs:31-54 without the BMP encoder): images[b] = host RGB bytes [heights[b]][widths[b]][3]; out_hwc_u8 = host
 * [batch][out_h][out_w][3].  One launch per pass for each sub-batch, mixed sizes included. */
int mse_resize_rgb8(const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, int batch, int out_w, int out_h, int filter,
                    uint8_t* out_hwc_u8);
/* Decoded images of any size in, features out (src/common.rs:31-54 + clip_server.py:131-146): upload, both passes, x / 127.5 - 1 and
 * the fp16 rounding fused into the vertical pass, which writes the tower's input buffer, then the forward pass.  Equal to
 * mse_resize_rgb8 to (img_size, img_size) followed by mse_siglip_encode_rgb8, bit for bit. */
int mse_siglip_encode_rgb8_any(mse_siglip* m, const uint8_t* const* images, const uint32_t* widths, const uint32_t* heights, int batch, int filter,
                               int normalize, float* out_f32, uint16_t* out_f16);
/* The same from 24-bit uncompressed BMP files of any size (src/common.rs:31-54; header check: mse_bmp24_info): the pixel arrays go up
 * as they are -- blue-green-red order, bottom-up rows and the 4-byte row padding are a matter of the kernels' source descriptor, there
 * is no host decode.  Equal to decoding with PIL followed by mse_siglip_encode_rgb8_any, bit for bit. */
int mse_siglip_encode_bmp_any(mse_siglip* m, const uint8_t* const* bmps, const size_t* sizes, int batch, int filter, int normalize,
                              float* out_f32, uint16_t* out_f16);
/* test hook (src/common.rs:31-54): the fp16 NCHW tower input [batch][3][img_size][img_size] the last _any call of this engine wrote */
int mse_debug_siglip_resize_nchw(mse_siglip* m, int batch, uint16_t* out);
/* measurement hook (scripts/resize_probe.py; src/common.rs:31-54): HIP-event milliseconds of the last resize of any kind in this
 * process, summed over its sub-batches: ms[0] upload, ms[1] horizontal pass, ms[2] vertical pass, ms[3] their sum */
int mse_resize_timing(double* ms);
const void* mse_siglip_output_device(const mse_siglip* m, int which);  /* device result of the last call: 0 f32, 1 f16 */
void* mse_siglip_stream(const mse_siglip* m);
int mse_siglip_debug_residual(mse_siglip* m, float* out);             /* test hook: residual stream after the last block */
int mse_debug_gemm_ms(int M, int N, int K, int ablation, int iters, float* ms_out); /* developer hook: GEMM timing/ablation */
/* developer / test hook for the small-batch GEMM kernels of the towers (one image, a few texts): `rows` real rows, bias (epi 0) or
 * bias + GELU (epi 1) epilogue, run by `variant` (0 = large-batch kernels, 1 = chosen by size, 2 = K-split skinny, 3 = 64 x 64 tiles,
 * 4 = 128 x 128 tiles).  ms_out = average launch time with weights streaming from HBM; n_diff (optional, TWO words) = output
 * elements that differ from the large-batch kernels' result, and those more than two bf16 steps apart (the kernels differ in
 * summation order only: the second word must be 0). */
int mse_debug_gemm_small(int rows, int N, int K, int epi, int variant, int iters, float* ms_out, uint64_t* n_diff);
/* test hooks for the towers' attention kernels alone (head width 72), through the launchers the towers call, so the tiling is chosen
 * from (B, heads, tokens) as in a forward pass.  Self attention: q / k / v host fp32 [B][heads][tokens][72], rounded to bf16 (nearest
 * even) and laid out as the QKV epilogue leaves them (token stride = tokens rounded up to 32, padding zero); out host fp32
 * [B][tokens][heads * 72] (the bf16 result widened).  flags bit 0: the padding (K rows, q rows and V columns from `tokens` to the
 * stride) holds finite garbage of magnitude up to 1e4 instead of zeros -- the result must not change.
 * Pooling attention (MAP head): qlat host fp32 [heads * 72], k / v host fp32 [B][tokens][heads * 72] (rounded to bf16); out host fp32
 * [B][heads * 72]. */
int mse_debug_siglip_attention(const float* q, const float* k, const float* v, int B, int heads, int tokens, int flags, float* out);
int mse_debug_siglip_pool_attention(const float* qlat, const float* k, const float* v, int B, int heads, int tokens, float* out);
/* test hooks for the towers' GEMM launches alone: ONE launch_gemm call (or the launch_ln_fold / launch_row_stats / launch_gemm_fused /
 * launch_ln_finalize sequence of the LayerNorm-fused path) filled in as the towers fill it in, so the kernel is chosen from
 * (epi, rows, N, K, skinny) as in a forward pass.  Operands are host fp32, rounded in the hook (nearest even) to the 16-bit type the
 * towers hold them in; destinations come back WHOLE -- M = rows rounded up to 256 rows, padding included -- widened to fp32.  Every
 * destination lies between guard bands and is filled with bytes 0xA5 before the launch (bf16 0xA5A5 = -7.17e-16, fp16 0xA5A5 =
 * -0.02204, fp32 -2.87e-16): an element that still holds that value was not written, and a changed guard byte fails the call.  What
 * a launch may do to padding rows is written above the hooks in csrc/siglip_api.hip.  A geometry the launchers do not accept is
 * refused before anything runs.  A call with every output pointer NULL launches nothing and fills in the sizes. */
typedef struct mse_debug_siglip_gemm_args {
    int rows, N, K;          /* rows = m_valid; x has M = rows rounded up to 256 rows */
    int epi;                 /* 0 BF16, 1 GELU, 2 RESID, 3 PATCH, 4 QKV, 6 PART (K split: raw fp32 slabs) */
    int skinny;              /* GemmLaunch::skinny: 0 large-batch kernels, 1 by size, 2 / 3 / 4 force K-split skinny / 64 x 64 / 128 x 128 */
    int gelu_tanh;
    int flags;               /* 1: finite garbage (|v| <= 1e4) in x rows rows .. M; 2: in w rows n_valid .. N; 4: 128-column remainder on a side stream */
    int n_valid;             /* flags & 2 */
    int tokens, heads, dh;   /* PATCH: tokens (rows of pos); QKV: heads, dh = 72, tokens (the row stride is tokens rounded up to 32) */
    int ksplit;              /* PART */
    const float *x, *w, *bias;   /* [rows][K], [N][K] (rows < n_valid are read), [N] */
    const float* resid;      /* RESID: fp32 [rows][N] */
    const float* pos;        /* PATCH: fp32 [tokens][N] */
    float* out;              /* BF16 / GELU (bf16), PATCH (fp16), RESID (fp32): [M][N]; PART: [ksplit][slab_rows][N] */
    float *q, *k, *vt;       /* QKV: [n_seq * heads][n_pad][dh_pad], [n_seq * heads][n_pad][kdh_pad], [n_seq * heads][dv_pad][n_pad] */
    int M, n_pad, n_seq, dh_pad, kdh_pad, dv_pad, slab_rows, cu_count;   /* filled in by the hook (cu_count only by a call that runs) */
} mse_debug_siglip_gemm_args;
int mse_debug_siglip_gemm(mse_debug_siglip_gemm_args* args);
typedef struct mse_debug_siglip_gemm_fused_args {
    int rows, N, K;          /* consumers: K = D, the width of the residual stream */
    int epi;                 /* 4 QKV, 1 GELU (consumers of a LayerNorm); 5 RESID_LN (producer) */
    int gelu_tanh;
    int flags;               /* 1: garbage in the padding rows of x (and xres); 2 (producer): in w rows n_valid .. N */
    int n_valid;             /* producer: real columns; N = n_valid rounded up to 256 */
    int heads, dh, tokens;   /* QKV */
    float eps;
    const float* x;          /* consumers: fp16 residual [rows][K]; producer: bf16 branch input [rows][K] */
    const float *w, *bias;   /* bf16 [N][K], fp32 [N] */
    const float *gamma, *beta;   /* consumers: fp32 [K] */
    const float* xres;       /* producer: fp16 residual [rows][n_valid] */
    float* out;              /* GELU: bf16 [M][N]; producer: the updated fp16 residual [M][n_valid] */
    float *q, *k, *vt;       /* QKV, as above */
    float* stats;            /* (mean, 1/std) [M][2]: row_stats (consumers), ln_finalize of the producer's parts */
    int M, n_pad, n_seq, dh_pad, kdh_pad, dv_pad;   /* filled in by the hook */
} mse_debug_siglip_gemm_fused_args;
int mse_debug_siglip_gemm_fused(mse_debug_siglip_gemm_fused_args* args);
/* test hooks for the towers' row kernels alone: each call makes ONE call of the launcher the towers use (launch_layernorm_d,
 * launch_patchify, launch_rgb8_to_nchw_f16, launch_bmp24_to_nchw_f16, launch_embed_tokens, launch_f32_to_bf16_pad,
 * launch_small_linear, launch_l2norm, launch_vt_ones_row), with the contract of the GEMM hooks.  Operands are host fp32 (u8 for the
 * decoders, i64 for tokens), compact -- [rows][width] -- and are rounded in the hook (nearest even) to the type the towers hold them
 * in and laid out with the leading dimension given (operand columns past the width hold 1e4).  Every destination -- the x that
 * LayerNorm updates in place included -- lies between guard bands, is filled with bytes 0xA5 before the launch and comes back WHOLE,
 * [rows][leading dimension], widened to fp32; a changed guard byte fails the call.  A geometry the launcher refuses is refused
 * before anything is allocated.  What each launch writes is stated above the hooks in csrc/siglip_api.hip. */
typedef struct mse_debug_siglip_layernorm_args {
    int rows, width;
    int ldx, x_is_f16;       /* x: rows of ldx elements, fp16 (the residual stream) or fp32 */
    int ldd;                 /* delta */
    int n_parts, part_rows, ldp;   /* parts: n_parts slabs of part_rows rows of ldp */
    int ldo;                 /* out and out_f32 */
    int wg;                  /* launch_layernorm_d's wg: 1 = layernorm_wg_kernel (a workgroup per row), 0 = layernorm_kernel (a wave per row) */
    float eps;
    const float* x;          /* [rows][width] */
    const float* delta;      /* optional: bf16 [rows][width] */
    const float* parts;      /* optional: fp32 [n_parts][rows][width], with bias fp32 [width] */
    const float* bias;
    const float *gamma, *beta;   /* fp32 [width] */
    float* x_out;            /* x after the call, [rows][ldx] */
    float* out;              /* optional: bf16 [rows][ldo] */
    float* out_f32;          /* optional: fp32 [rows][ldo] */
} mse_debug_siglip_layernorm_args;
int mse_debug_siglip_layernorm(mse_debug_siglip_layernorm_args* args);
/* img fp32 [B][C][H][W] (rounded to fp16 when is_f16); out bf16 [B * tstride][k_pad] */
int mse_debug_siglip_patchify(const float* img, int is_f16, int B, int C, int H, int W, int P, int k_pad, int tstride, float* out);
/* in u8 [B][H][W][C]; out fp16 [B][C][H][W] */
int mse_debug_siglip_rgb8(const uint8_t* in, int B, int C, int H, int W, float* out);
/* in: B BMP pixel arrays img_stride bytes apart, rows of row_stride bytes (BGR); flags[b] bit 0 = bottom row first; out fp16 [B][3][H][W] */
int mse_debug_siglip_bmp24(const uint8_t* in, size_t img_stride, int row_stride, const uint8_t* flags, int B, int H, int W, float* out);
/* tokens i64 [rows], tok_emb fp32 [vocab][D], pos fp32 [ctx][D]; out fp16 [rows][D] */
int mse_debug_siglip_embed_tokens(const int64_t* tokens, const float* tok_emb, const float* pos, int vocab, int ctx, int D, int rows, float* out);
/* in fp32 [rows][cols] (laid out with rows of ld_in); out bf16 [rows_pad][cols_pad] */
int mse_debug_siglip_f32_to_bf16_pad(const float* in, int rows, int cols, int ld_in, int rows_pad, int cols_pad, float* out);
/* x fp32 [B][K], w [N][K] (rounded to bf16), bias fp32 [N]; y fp32 [B][ldy] */
int mse_debug_siglip_small_linear(const float* x, int ldx, const float* w, int ldw, const float* bias, int K, int N, int B, int ldy, float* y);
/* x fp32 [B][width]; out_f32 / out_f16 (either may be NULL) [B][width] */
int mse_debug_siglip_l2norm(const float* x, int ldx, int width, int B, int normalize, float* out_f32, float* out_f16);
/* out: n_mats sentinel-filled bf16 [dv_pad][n_pad] matrices after launch_vt_ones_row */
int mse_debug_siglip_vt_ones_row(int n_mats, int dh, int dv_pad, int n_pad, float* out);

/* ---- SigLIP text tower: `model.encode_text(tokens)` + normalisation + fp16 serialisation
 * (clip_server.py:98-99,128-131,166).  open_clip's TextTransformer is a third-party dependency not vendored in
 * the reference; geometry from misc/clip_accursed.py:31-55 and clip_server.py:107,182: width 1152, 27 layers,
 * 16 heads, mlp 4304, context 64, vocabulary 32000, no causal mask, last position pooled, Linear projection with
 * bias.  Weight names are open_clip's (`text.token_embedding.weight`, `text.transformer.resblocks.N. ...`).
 * Every row is within 1e-3 cosine of the fp32 model and a call is deterministic; NO bit-equality of a text across call sizes
 * (or MSE_SIGLIP_TEXT_PARTS) is promised, and no tolerance between call sizes has been measured.
 * Tokenisation (sentencepiece, pad id 1, clip_server.py:129) stays on the host. */
typedef struct mse_siglip_text mse_siglip_text;
typedef struct mse_siglip_text_config {
    int width;           /* 1152 */
    int layers;          /* 27 */
    int heads;           /* 16 */
    int mlp_dim;         /* 4304 */
    int context_length;  /* 64 */
    int vocab_size;      /* 32000 */
    float eps;           /* 1e-6 */
    int gelu_tanh;       /* 0 erf, 1 tanh approximation */
    int max_batch;
} mse_siglip_text_config;
mse_siglip_text* mse_siglip_text_create(const mse_siglip_text_config* cfg);
void mse_siglip_text_destroy(mse_siglip_text* m);
int mse_siglip_text_n_weights(const mse_siglip_text* m);
const char* mse_siglip_text_weight_name(const mse_siglip_text* m, int idx);
int mse_siglip_text_set_weight(mse_siglip_text* m, const char* name, const float* data, const size_t* shape, int ndim);
int mse_siglip_text_finalize(mse_siglip_text* m);
/* tokens: host int64 [batch, context_length]; outputs (either may be NULL) are host [batch, width]. */
int mse_siglip_text_encode(mse_siglip_text* m, const int64_t* tokens, int batch, int normalize, float* out_f32,
                           uint16_t* out_f16);
/* The same forward with the features left ON THE DEVICE, nothing copied back and nothing waited for: the request handler embeds the
 * query text (src/query_disk_index.rs:345-381) and searches with it (:436-540) -- order the searcher behind the engine's stream
 * (mse_searcher_wait_stream(s, mse_siglip_text_stream(m))) and pass mse_siglip_text_output_device(m, 1) as the device-resident f16
 * queries of mse_disk_query_topk.  `tokens` (host) must stay untouched until the engine's stream has read them; the output buffers
 * (which: 0 = f32 [batch][width], 1 = f16) belong to the engine and hold this call's rows until its next call. */
int mse_siglip_text_encode_dev(mse_siglip_text* m, const int64_t* tokens, int batch, int normalize);
const void* mse_siglip_text_output_device(const mse_siglip_text* m, int which);
void* mse_siglip_text_stream(const mse_siglip_text* m);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* MSE_H */
