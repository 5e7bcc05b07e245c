// Internal launch interface between the translation units of libmse_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mse {

constexpr uint32_t ID_NONE = 0xFFFFFFFFu;
constexpr int TOPK_KMAX = 2048;    // largest k (incl. margin) one selection can return
constexpr int TOPK_FANOUT = 256;   // children per tournament group
constexpr int GROUP_ROWS = 32;     // base rows per group maximum written by the MFMA scan (64 on the 320-query pass: mfma_group_rows)

// ---- scan_exact.hip ------------------------------------------------------------------------
// ids != nullptr (filtered search): score rows ids[0 .. n_rows) instead of rows 0 .. n_rows; scores stay at the list positions
int launch_scan_exact(const uint16_t* base, size_t n_rows, int d, const void* queries_dev, int nq, bool q_is_f32,
                      int64_t* scores, size_t score_stride, float* fscores, int n_cu, hipStream_t stream, const uint32_t* ids = nullptr);
int launch_score_rows(const uint16_t* base, size_t n_rows, int d, const void* queries_dev, bool q_is_f32,
                      const uint32_t* ids_dev, size_t n_pairs, size_t pairs_per_query, int64_t* out, float* fout,
                      hipStream_t stream);

// ---- gen.hip ---------------------------------------------------------------------------------
int launch_generate_rows(uint16_t* out, uint32_t seed, uint64_t row0, size_t n_rows, int d, hipStream_t stream);
// *out_max_norm_bits = max over rows of ||row||_2 (float bits, atomicMax on non-negative floats); zero it first
int launch_row_norm_max(const uint16_t* base, size_t n_rows, int d, uint32_t* out_max_norm_bits, hipStream_t stream);
// eps[q] = factor * ||query_q||_2 * max_norm   (queries f16 [nq][d])
int launch_query_eps(const uint16_t* queries, int nq, int d, const uint32_t* max_norm_bits, float factor, float* eps,
                     hipStream_t stream);

// the same for f32 queries scanned as their f16 roundings q16: adds |q32 - q16| * max_norm (flat index)
int launch_query_eps_f32(const float* q32, const uint16_t* q16, int nq, int d, const uint32_t* max_norm_bits, float factor, float* eps,
                         hipStream_t stream);

// ---- topk.hip --------------------------------------------------------------------------------
enum KeyKind { KEY_I64 = 0, KEY_F32 = 1, KEY_U64 = 2, KEY_U32 = 3 };
// out[q][g] = max over in[q][g*F .. (g+1)*F) as order-preserving unsigned keys
// (u64 keys for KEY_I64/KEY_U64 input, u32 keys for KEY_F32/KEY_U32 input).
int launch_reduce_max(KeyKind kind, const void* in, size_t in_stride, size_t n_in, void* out, size_t out_stride,
                      size_t n_out, int nq, hipStream_t stream, size_t in_estride = 1);   // element (q, i) at in[q*in_stride + i*in_estride]
struct SelectArgs {
    KeyKind kind;            // type of `in` / `list_keys`
    const void* in;          // level array, [nq][in_stride]
    size_t in_stride, n_in;
    const uint32_t* parents; // [nq][par_stride] group ids (ID_NONE = empty), or nullptr
    size_t par_stride, n_par;
    int fanout;              // children per parent
    const uint32_t* list_ids;  // explicit candidates [nq][list_stride] (with list_keys), or nullptr
    const void* list_keys;
    size_t list_stride, n_list;
    size_t list_chunk = 0, list_chunk_stride = 0;  // if list_chunk != 0: candidate c lives at (c / chunk) * chunk_stride + c % chunk
    size_t list_id_chunk_stride = 0;               // chunk stride of list_ids when it differs from that of list_keys (0 = the same)
    const uint32_t* list_count = nullptr;          // optional, per query: only the first min(list_count[q], n_list) candidates exist
    int k;                   // number to select (<= TOPK_KMAX)
    uint32_t* out_ids;       // [nq][out_stride], best first, padded with ID_NONE
    void* out_keys;          // optional: raw keys (same type as `in`) of the selected, [nq][out_stride]
    size_t out_stride;
    int nq;
    // optional, per query, in the composite's score domain (sortable u64; 32-bit keys sit in the top half):
    // floor_hi: candidates whose score key is below it are skipped (the caller knows >= k candidates reach it -- e.g. the
    // k-th best key of the parent level, since every one of the k best parents has a child with exactly its key);
    // kth_hi_out: receives a lower bound of the score key of the k-th best candidate that at least k candidates reach -- the key
    // itself, or the key with its low digits zeroed when the radix search ended early (0 when no more than k candidates exist).
    const unsigned long long* floor_hi = nullptr;
    unsigned long long* kth_hi_out = nullptr;
};
int launch_select(const SelectArgs& a, hipStream_t stream);
// same, with element (q, i) of `in` at in[q*in_stride + i*in_estride] (group-major level arrays)
int launch_select_strided(const SelectArgs& a, size_t in_estride, hipStream_t stream);
// group-major float level [n_in][nq_pad] -> query-major u32 keys [nq][out_stride]
int launch_reduce_max_gq(const float* in, int nq_pad, size_t n_in, uint32_t* out, size_t out_stride, size_t n_out,
                         int nq, hipStream_t stream);
// ids[q][p*group + r] = parents[q][p]*group + r (ID_NONE if parent empty or row >= n_rows)
int launch_expand_groups(const uint32_t* parents, size_t par_stride, size_t n_par, int group, size_t n_rows,
                         uint32_t* ids, size_t ids_stride, int nq, hipStream_t stream);
// final packaging: out_scores[q][i] = keys (i64) ; out_ids[q][i] = ids + id_offset ; certificate margin
int launch_finalize(const uint32_t* sel_ids, const int64_t* sel_scores, size_t sel_stride, int k, int nq,
                    uint64_t id_offset, int64_t* out_scores, uint32_t* out_ids, size_t out_stride,
                    const float* group_keys, size_t gk_stride, int kg, size_t n_groups, const float* eps,
                    float* margin, hipStream_t stream, const float* tau = nullptr /* per query: the bound is max(worst chosen key, tau) */);

// Thresholded group maxima (bruteforce.hip mfma_pass, the sparse form of the 320-query pass).  counts [nq_pad], ids / keys [nq_pad][cap].
// tau[q] = the next float below gk[q][k - 1] - 3 eps[q] for q < nq (gk: the k best sample maxima, best first), +inf for the padding
// columns up to nq_pad; counts[0 .. nq_pad) = 0
int launch_sparse_tau(const float* gk, size_t gk_stride, int k, const float* eps, int nq, int nq_pad, float* tau, uint32_t* counts, hipStream_t stream);
// the sample's survivors: entry (sg, q) of the sample's dense maxima [n_sg][nq_pad] above tau[q] is appended to list q as group
// (sg / 4) * 4 * stride + sg % 4 (the sample is every stride-th 256-row tile = four 64-row groups)
int launch_sparse_append_sample(const float* dense, int nq_pad, size_t n_sg, int nq, uint32_t stride, const float* tau, uint32_t* counts,
                                uint32_t* ids, float* keys, uint32_t cap, hipStream_t stream);
// lists, counts (clamped to cap) and thresholds of the queries idx[0 .. nb) as a compact set
int launch_sparse_gather_lists(const uint32_t* ids, const float* keys, const uint32_t* counts, const float* tau, uint32_t cap, const uint32_t* idx,
                               int nb, uint32_t* out_ids, float* out_keys, uint32_t* out_counts, float* out_tau, hipStream_t stream);

// certificate margin for f32 keys: margin[q] = sel_keys[q][k-1] - (group_keys[q][kg-1] + eps[q])   (flat index)
int launch_margin_f32(const uint32_t* sel_ids, const float* sel_keys, size_t sel_stride, int k, int nq, const float* group_keys,
                      size_t gk_stride, int kg, size_t n_groups, const float* eps, float* margin, hipStream_t stream);

// per-query widening helpers: out[g][j] = in[g][idx[j]] (j < nb; -inf in the padding columns) | out row j = in row idx[j] (rows of
// row_bytes, a multiple of 16) | dst row idx[j] = src row j for the j with take[j] != 0 (take == nullptr: all)
int launch_gather_columns(const float* in, int nq_pad, size_t n_groups, const uint32_t* idx, int nb, float* out, int nbp, hipStream_t stream);
int launch_gather_rows16(const void* in, size_t row_bytes, const uint32_t* idx, int nb, void* out, hipStream_t stream);
int launch_scatter_topk(const uint32_t* idx, const uint8_t* take, int nb, int k, const int64_t* src_s, const uint32_t* src_i, int64_t* dst_s,
                        uint32_t* dst_i, size_t dst_stride, hipStream_t stream);

// a shard's [n] results on their way into a packed block: out_sc[i] = sc[i], out_ids[i] = ids[i] + id_offset; empty slots (ID_NONE, or
// sc == nullptr) become (INT64_MIN, ID_NONE)
int launch_block_finish(const int64_t* sc, const uint32_t* ids, size_t n, uint64_t id_offset, int64_t* out_sc, uint32_t* out_ids, hipStream_t stream);
int launch_scatter_rows4(const uint32_t* idx, const uint8_t* take, int nb, int k, const void* src, void* dst, size_t dst_stride, hipStream_t stream);

// ---- pq.hip ----------------------------------------------------------------------------------
int launch_pq_transform(const float* T, int d, const float* x, size_t n, float* out, hipStream_t stream);
int launch_pq_transform_vec(const float* T_transposed, int d, const float* x, float* out, hipStream_t stream);   // n = 1, same arithmetic
int launch_pq_lut(const float* centroids, int n_centroids, int d, int dpc, const float* t, float* lut,
                  hipStream_t stream);
int launch_pq_quantize(const float* centroids, int n_centroids, int d, int dpc, const float* t, size_t n,
                       uint8_t* codes, hipStream_t stream);
// nq > 1 (gathered ids only): query y uses table lut + y * n_chunks * n_centroids, ids + y * q_stride, out + y * q_stride
int launch_pq_adc(const float* lut, int n_chunks, int n_centroids, const uint8_t* codes, size_t n_codes,
                  const uint32_t* ids, size_t n, const uint8_t* desc, int n_desc, const float* scales, int64_t* out,
                  int n_cu, hipStream_t stream, int nq = 1, size_t q_stride = 0);
bool pq_scan_gmax_supported(int n_chunks, int n_centroids, const uint8_t* desc, int n_desc, const float* scales);
// mask (all three group-maximum scans): the bitmap words of an mse_filter -- the masked instantiation, where a vector whose bit is clear
// (or at / past 32 * mask_words) counts like one past the end of the codes; null: the unfiltered kernel, launched exactly as ever
int launch_pq_scan_gmax(const float* lut, const uint8_t* codes, size_t n, const uint8_t* desc, const float* scales,
                        int64_t* gmax, int n_cu, hipStream_t stream, const uint32_t* mask = nullptr, size_t mask_words = 0);
int launch_pq_scan_gmax2(const float* lut0, const float* lut1, const uint8_t* codes, size_t n, const uint8_t* desc,
                         const float* scales, int64_t* gmax0, int64_t* gmax1, int n_cu, hipStream_t stream, const uint32_t* mask = nullptr,
                         size_t mask_words = 0);
// four queries per pass: 12-bit integer nomination tables + certificate (pq.hip)
struct Pq4Params { double delta, c, eps; int ok; };
size_t pq4_table_bytes();
int launch_pq4_table(const float* luts, const float* scales, int n_valid, void* table, Pq4Params* params, hipStream_t stream, int nq = 4);
int launch_pq_scan_gmax4(const void* table, const uint8_t* codes, size_t n, const uint8_t* desc, uint32_t* gmax, int n_cu,
                         hipStream_t stream, int nq = 4,    // nq = 4: 12-bit tables, 8: 8-bit tables; gmax [n_groups][nq] (group-major)
                         const uint32_t* mask = nullptr, size_t mask_words = 0);
int launch_pq4_certify(const Pq4Params* params, const uint32_t* group_keys, int n_nominated, int n_sel, const uint32_t* top_ids,
                       const int64_t* top_scores, size_t top_stride, int r, int nq, int* flag, hipStream_t stream);
int launch_add_descriptor(const uint32_t* ids, size_t n, const uint8_t* desc, int n_desc, size_t n_codes,
                          const float* scales, int64_t* out, hipStream_t stream);
int launch_f32_to_f16(const float* in, size_t n, uint16_t* out, hipStream_t stream);
int launch_f16_to_f32(const uint16_t* in, size_t n, float* out, hipStream_t stream);
int launch_pq_lut_batch(const float* centroids, int n_centroids, int d, int dpc, const float* t, size_t nq, float* lut,
                        hipStream_t stream);
int rank_max_targets();
int launch_rank(const int64_t* scores, size_t n, const uint32_t* targets, int m, unsigned long long* counts, int n_cu,
                hipStream_t stream);

// ---- pq_train.hip: codec training (include/mse.h mse_pq_trainer) ----------------------------------------------------
// *max_bits = bit pattern of max |v| over count floats (zeroed here first); inf / NaN patterns win the maximum
int launch_abs_max(const float* v, size_t count, uint32_t* max_bits, hipStream_t stream);
// *E = 61 - ceil(log2 n) - ex for vmax = f 2^ex, f in [0.5, 1) (ex = 0 at vmax = 0); a non-finite maximum sets bit 0 of *err instead
int launch_fixed_exponent(const uint32_t* max_bits, size_t n, int* E, uint32_t* err, hipStream_t stream);
// The order-free sum: slice z < n_slices adds llrint((double)v[row][z * v_step + c] * 2^E) for c < w into sums[z * sums_step + cell * w + c],
// cell = code[row * code_stride + z * code_step] (a code at or past n_cells is skipped), as int64 through integer atomics.  sums (and
// counts, optional: members per cell, [n_slices][n_cells]) are zeroed by the caller.  The result does not depend on rows_per_block (0: 4096)
struct AccumulateArgs {
    const float* v = nullptr; size_t n = 0; int w = 0; size_t v_stride = 0; int v_step = 0;
    const uint8_t* code = nullptr; size_t code_stride = 1; int code_step = 0;
    int n_cells = 0, n_slices = 1; const int* E = nullptr;
    long long* sums = nullptr; size_t sums_step = 0;
    unsigned long long* counts = nullptr;
    unsigned rows_per_block = 0;
};
int launch_accumulate_by_code(const AccumulateArgs& a, hipStream_t stream);
// centroids[k][s * dpc + u] = (float)(((double)sums[s][k][u] / (double)counts[s][k]) * 2^-E); a cell with count 0 is left alone and adds 1 to *empty
int launch_kmeans_update(const long long* sums, const unsigned long long* counts, const int* E, int n_chunks, int n_cells, int dpc, int d,
                         float* centroids, unsigned long long* empty, hipStream_t stream);
// G [n][d] = R Cm with R = xr - (the centroids the codes name), formed while the operand is loaded; G may be null (loss only).
// lrow [n] = r . G_row; lpart: scratch of n * residual_gemm_parts(d) floats.  Every output is one k-ascending fma chain
int residual_gemm_parts(int d);
int launch_residual_gemm(const float* xr, const uint8_t* codes, const float* centroids, const float* Cm, size_t n, int d, int dpc, float* G,
                         float* lpart, float* lrow, hipStream_t stream);
int launch_loss_finish(const long long* S, const int* E, size_t n, double* out, hipStream_t stream);   // *out = ((double)S 2^-E) / n
// gradient from the chunk sums (sums + c * slot_stride with exponent E[c], c < n_slots, layout [n_chunks][n_cells][dpc]) and one Adam step
struct AdamArgs {
    const long long* sums; size_t slot_stride; const int* E; int n_slots; size_t n;
    int n_chunks, n_cells, dpc, d;
    float *centroids, *m, *v, *grad;   // grad [n_cells][d]: the step's gradient, kept for mse_pq_trainer_gradient
    float beta1, beta2, step_size, bc2_sqrt, eps;
};
int launch_adam_step(const AdamArgs& a, hipStream_t stream);
// M [d][d] f64 from the full-width sums sigma [n_chunks][n_cells][d] of X' by each sub-space's codes
int launch_cross_matrix(const long long* sigma, const int* E, const float* centroids, int n_cells, int dpc, int d, double* M, hipStream_t stream);
int launch_transpose_f32(const float* in, int d, float* out, hipStream_t stream);
int launch_gather_rows_f16(const uint16_t* base, const uint32_t* ids, size_t n, int d, uint16_t* out, hipStream_t stream);

// ---- partition.hip: the shard partition (include/mse.h mse_partitioner) ----------------------------------------------
// One pass rows x centroids: score(x, c) = the k-ascending f64 chain over exact products.  Row r < n is rows[ids ? ids[r] : r].  Whatever of
// sizes ([2][S], added to; rank 0 = best centroid of a row, rank 1 = second; f64 score descending, lowest index on ties), top2 ([n][2]) and
// scores ([n][S]) is not null is written.  stopped (optional): a non-zero word makes the launch a no-op
struct PartitionScoreArgs {
    const uint16_t* rows = nullptr; const uint32_t* ids = nullptr; size_t n = 0; int d = 0, S = 0;
    const float* cen = nullptr;
    unsigned long long* sizes = nullptr; uint8_t* top2 = nullptr; double* scores = nullptr;
    const uint32_t* stopped = nullptr;
};
int launch_partition_score(const PartitionScoreArgs& a, hipStream_t stream);
// the annealing state on the device: mse_partition_status (include/mse.h) and, after it, which of the two centroid buffers is current
struct PartitionDevState {
    unsigned long long t, last, li;
    float T; uint32_t stopped;
    uint32_t cur, pad;
};
struct PartitionAnnealArgs {
    PartitionDevState* st; float* c[2]; float* nrm;        // raw centroids (two buffers [S][d]), the normalised candidate
    unsigned long long* sizes;                             // [2][S]: read by the decision, zeroed by it for the next count
    unsigned long long* trace_F; uint8_t* trace_code; size_t trace_cap;   // entry t - 1 belongs to iteration t >= 1
    int S, d; size_t n;
    uint32_t seed, reroll_after;
    float accept_decay, reject_decay, reroll_heat, cap;
    unsigned long long stop_num, stop_den;                 // stop when last * stop_den < n * stop_num
};
// candidate of iteration st->t into c[cur ^ 1] (t = 0: the initial noise; else c[cur] + z T) and its normalisation into nrm
int launch_partition_candidate(const PartitionAnnealArgs& a, hipStream_t stream);
// the decision of iteration st->t from sizes (include/mse.h); the rerolled rows are rewritten by the same launch
int launch_partition_decide(const PartitionAnnealArgs& a, hipStream_t stream);
// out = the rows of c normalised; f16_out (RNE of out) and wide_out (f16_out widened) may be null
int launch_partition_normalise(const float* c, int S, int d, float* out, uint16_t* f16_out, float* wide_out, hipStream_t stream);
int launch_partition_noise(uint32_t seed, uint64_t key, int d, float* out, hipStream_t stream);   // z(key), d floats
// dump_processor.rs:438-461 over `rows` rows of scores [rows][S]: one wave, lane = shard; counts [S] and *bal carry on from call to call
int launch_partition_walk(const double* scores, size_t rows, int S, double fudge, unsigned long long* counts, unsigned long long* bal,
                          uint8_t* assignment, hipStream_t stream);
// bit r of bits = row r of assignment [n][2] names shard s; bits holds whole 64-row words
int launch_partition_shard_bits(const uint8_t* assignment, size_t n, int s, uint32_t* bits, hipStream_t stream);

// ---- disk_search.hip: the runtime de-duplication of the request path for a batch, on the device ------------------------------------
// per query q: similarity bits over its visited records (vis_ids [nq][cap], n_visited[q] of them, visit order), greedy keep-first
// filter; a dropped record becomes (ID_NONE, INT64_MIN) in place.  bits: dedup_batch_scratch_bytes(nq, cap) bytes of scratch.
size_t dedup_batch_scratch_bytes(size_t nq, size_t cap);
int launch_dedup_batch(const uint16_t* base, int d, uint32_t* vis_ids, long long* vis_scores, size_t cap, const uint32_t* n_visited, size_t nq,
                       float threshold, void* bits, hipStream_t st);
// ---- filter.hip: row filters of the filtered brute-force search -------------------------------------------------------------
// words: n_words zeroed bitmap words; sets the bit of each of the n ids (all < 32 * n_words)
int launch_filter_or_ids(uint32_t* words, size_t n_words, const uint32_t* ids, size_t n, hipStream_t stream);
// the ids of the set bits, ascending, into ids_out (room for every set bit); *count_dev = how many.  scratch: filter_compact_scratch_bytes
size_t filter_compact_scratch_bytes(size_t n_words);
int launch_filter_compact(const uint32_t* words, size_t n_words, uint32_t* ids_out, unsigned long long* count_dev, void* scratch,
                          hipStream_t stream);
// launch_filter_compact in two steps, for an id list sized by the count: *count_dev = set bits and the block offsets into scratch
// (filter_compact_scratch_bytes), then -- same words, same scratch -- the ascending ids into ids_out (room for *count_dev of them)
int launch_filter_count(const uint32_t* words, size_t n_words, unsigned long long* count_dev, void* scratch, hipStream_t stream);
int launch_filter_write_ids(const uint32_t* words, size_t n_words, const void* scratch, uint32_t* ids_out, hipStream_t stream);
// Filters as values.  Each writes all n_words words of `out` (whole 256-row tiles over n_rows) and no bit at or past n_rows.
// out = a OP b (op: MSE_FILTER_AND / OR / XOR / ANDNOT; 4 = NOT a, b unused); an operand reads as zero at and past its own words
int launch_filter_combine(const uint32_t* a, size_t a_words, const uint32_t* b, size_t b_words, int op, size_t n_rows, size_t n_words,
                          uint32_t* out, hipStream_t stream);
// bit r = byte j of lo <= desc[r][j] <= byte j of hi for every j < n_desc (1 .. 8)
int launch_filter_desc_range(const uint8_t* desc, int n_desc, size_t n_rows, uint64_t lo, uint64_t hi, size_t n_words, uint32_t* out,
                             hipStream_t stream);
// bit r = scores[r] >= threshold AND bit r of within (null: every row; zero at and past within_words)
int launch_filter_score_threshold(const int64_t* scores, size_t n_rows, int64_t threshold, const uint32_t* within, size_t within_words,
                                  size_t n_words, uint32_t* out, hipStream_t stream);
// clears the bits at and past n_rows in the word that holds row n_rows
int launch_filter_mask_tail(uint32_t* words, size_t n_rows, hipStream_t stream);
// out (n_words words, whole tiles over n_rows) = rows first_row .. first_row + n_rows of `in`, which reads as zero at and past its in_words
// words and its in_rows rows (mse_filter_slice)
int launch_filter_slice(const uint32_t* in, size_t in_words, size_t in_rows, uint64_t first_row, size_t n_rows, size_t n_words, uint32_t* out,
                        hipStream_t stream);
// out (a zero-initialised bitmap over n_rows rows) |= part (part_rows rows) at row first_row; a part past n_rows is an error.  The parts of
// one bitmap go on ONE stream, one launch each: parts sharing a boundary word then need no atomics (mse_filter_concat)
int launch_filter_place(const uint32_t* part, size_t part_rows, uint64_t first_row, size_t n_rows, uint32_t* out, hipStream_t stream);
// launch_expand_groups, with ID_NONE for rows whose bit is clear (or at / past 32 * n_words)
int launch_expand_groups_masked(const uint32_t* parents, size_t par_stride, size_t n_par, int group, size_t n_rows, const uint32_t* words,
                                size_t n_words, uint32_t* ids, size_t ids_stride, int nq, hipStream_t stream);
// out[w] = NOT deleted[w] below n_rows (deleted null: all ones), zero at and past n_rows: a graph's live rows as a filter bitmap of n_words words
int launch_filter_live(const uint32_t* deleted, size_t n_rows, size_t n_words, uint32_t* out, hipStream_t stream);
// sel[i] = list[sel[i]] (ID_NONE stays): positions in the filter's id list -> row ids
int launch_map_positions(uint32_t* sel, size_t n, const uint32_t* list, hipStream_t stream);
// out[w] = words[w] AND (has_url != 0 for the word's 32 rows; rows at or past n_rows excluded): the rows a filtered LIST search may return
int launch_filter_and_flags(const uint32_t* words, size_t n_words, const uint8_t* has_url, size_t n_rows, uint32_t* out, hipStream_t stream);
// scores[j * stride + p] += descriptor_product(scales + j * n_desc, row ids[p]) for j < nq <= 8, p < n (i64, per-term truncation)
int launch_list_bias(const uint32_t* ids, size_t n, const uint8_t* desc, int n_desc, const float* scales, int nq, int64_t* scores, size_t stride,
                     hipStream_t stream);

// ---- group.hip: row groupings of the grouped search (include/mse.h mse_groups) ---------------------------------------------------
// stats (three zeroed u64): [0] = largest non-NONE id + 1 (0: none), [1] = NONE rows; present (zeroed, (n_rows + 31) / 32 words): the bit
// of every id below n_rows.  An id at or past n_rows sets no bit
int launch_groups_validate(const uint32_t* group_of, size_t n_rows, uint32_t* present, unsigned long long* stats, hipStream_t stream);
// stats[2] += set bits of present
int launch_groups_popcount(const uint32_t* present, size_t n_words, unsigned long long* stats, hipStream_t stream);
// Collapse of ranked id lists, one workgroup per query: ids [nq][ids_stride], best first, ID_NONE padding at the tail only, the first
// n_list <= 2048 entries read; groups by LOCAL row id (a row at or past g_len, or of group NONE, is a group of its own).
// kept_pos [nq][k]: list positions of the first k representatives (ID_NONE padded); n_reps [nq]: representatives in the whole list
int launch_collapse(const uint32_t* ids, size_t ids_stride, size_t n_list, const uint32_t* group_of, size_t g_len, int k, int nq,
                    uint32_t* kept_pos, uint32_t* n_reps, hipStream_t stream);
// the entries at kept_pos with their payload (key_bytes 8: i64, padding INT64_MIN; 4: f32, padding -FLT_MAX; ids + id_offset, padding
// ID_NONE) into row dst_rows[q] (null: q) of the outputs, for the queries with take[q] != 0 (null: all)
int launch_collapse_gather(const uint32_t* kept_pos, int k, const uint32_t* ids, size_t ids_stride, const void* keys, size_t keys_stride,
                           int key_bytes, int nq, uint64_t id_offset, const uint32_t* dst_rows, const uint8_t* take, void* out_keys,
                           uint32_t* out_ids, size_t out_stride, hipStream_t stream);
// Dense path over level 0 (scores [nq][stride], one key per list position p < n; row = list[p], or p without a list): the best row of
// every group by (key desc, row asc) through integer atomics into best [nq][g_len] u64 (+ best_id [nq][g_len] u32 for i64 keys; unused
// for f32), then every grouped row that is not its group's best drops to the lowest key (INT64_MIN / the all-ones f32 pattern) IN PLACE.
// n_sat [nq] (i64 only): representatives and ungrouped rows whose own score is INT64_MIN.  ev_mid (optional): recorded between the
// atomics and the demotion
int launch_dense_group_best(bool f32, void* scores, size_t stride, size_t n, const uint32_t* list, const uint32_t* group_of, size_t g_len, int nq,
                            unsigned long long* best, uint32_t* best_id, uint32_t* n_sat, hipStream_t stream, hipEvent_t ev_mid = nullptr);
// i64, after the selection over the demoted level 0 (sel_keys [nq][k]), its collapse (kept_pos [nq][k], n_reps) and the gather into the
// outputs: a query with fewer than k representatives and n_sat > 0 gets its saturated representatives, in id order, behind the others
int launch_dense_complete(const int64_t* scores, size_t stride, size_t n, const uint32_t* list, const uint32_t* group_of, size_t g_len,
                          const uint32_t* best_id, const uint32_t* n_sat, const uint32_t* kept_pos, const uint32_t* n_reps, const int64_t* sel_keys,
                          int k, int nq, uint64_t id_offset, const uint32_t* dst_rows, int64_t* out_scores, uint32_t* out_ids, size_t out_stride,
                          hipStream_t stream);
// The group step of the graph request path over UNRANKED visited lists (vis_ids / vis_scores [nq][cap], min(n_visited[q], cap) records,
// holes (ID_NONE, INT64_MIN) allowed anywhere): of every group the best live record by (score desc, id asc) stays, every other record of
// the group becomes a hole in place; records of group NONE or at / past g_len and entries past the list are not touched.  cap <= 4096: the
// table lives in LDS and `table` is not read; longer lists: visited_group_scratch_bytes(nq, cap) bytes of scratch, run in query chunks
size_t visited_group_scratch_bytes(size_t nq, size_t cap);
int launch_visited_group(uint32_t* vis_ids, long long* vis_scores, size_t cap, const uint32_t* n_visited, size_t nq, const uint32_t* group_of,
                         size_t g_len, void* table, hipStream_t stream);
// The same step over the gathered packed blocks of a sharded search, in place (the grouped merge, include/mse.h): n_shards blocks of
// {[nq][k_in] i64 scores, [nq][k_in] u32 GLOBAL ids}, block_bytes apart; group_of / g_len: the GLOBAL grouping, on the blocks' device.
// n_shards * k_in <= 4096 records per query: the table lives in LDS; more: merge_group_scratch_bytes(nq, n_shards * k_in) bytes of `table`
size_t merge_group_scratch_bytes(size_t nq, size_t n_records);
int launch_merge_group(void* blocks, size_t block_bytes, size_t n_shards, size_t nq, size_t k_in, const uint32_t* group_of, size_t g_len, void* table,
                       hipStream_t stream);
// mse_groups_slice's relabelling: labels [m] (each below the source's length, or NONE) -> out [m], the lowest i with the same label (NONE
// stays); table: scratch of the source's length in u32, uninitialised
int launch_groups_slice(const uint32_t* labels, size_t m, uint32_t* table, uint32_t* out, hipStream_t stream);

// ---- graph_build.hip: what graph_delete.hip shares with the build ---------------------------------------------------------------
// robust_prune (lib.rs:227-285), one workgroup per candidate list: list k is (ci, cs)[k * stride ..][0 .. counts[k]) in HBM, its point
// points[k]; the new list (at most r ids) goes to out_ids[k * r ..], its length to out_len[k].  eps_fix: prune_mfma_eps (runtime.h)
struct PruneLaunch {
    const uint16_t* base; uint32_t n; int d;
    uint32_t qb; long long alpha, qalpha; int r, maxc, saturate;
    long long eps_fix; uint32_t* err;   // err: one zeroed device word (bits 16 / 32: a candidate id outside the index)
};
int launch_prune_lists(const PruneLaunch& p, const uint32_t* ci, const long long* cs, size_t stride, const uint32_t* counts, const uint32_t* points,
                       uint32_t* out_ids, uint32_t* out_len, size_t nb, hipStream_t stream);
// list of points[k] = staged[k * r ..][0 .. staged_len[k]) (staged_len <= 64); the graph's lists have stride `stride` >= r
int launch_apply_lists(uint32_t* adj, uint32_t* deg, size_t stride, int r, const uint32_t* points, const uint32_t* staged, const uint32_t* staged_len,
                       size_t nb, hipStream_t stream);

// ---- graph_delete.hip: delete consolidation (include/mse.h mse_graph_delete_rows) -----------------------------------------------
// dbits: the delete set D, one bit per node (words as mse_filter keeps them).  All counters / error words are zeroed by the caller.
// affected[w] = the nodes of word w that are not in D and list a member of D; *err |= 1 for an edge outside the graph or a list longer
// than the stride; *n_new += members of D whose bit in `deleted` (may be null) is clear
int launch_delete_mark(const uint32_t* adj, const uint32_t* deg, size_t n, int stride, const uint32_t* dbits, const uint32_t* deleted,
                       uint32_t* affected, uint32_t* err, uint32_t* n_new, hipStream_t stream);
// *hit |= 1 if one of the ids is in D
int launch_delete_check_ids(const uint32_t* ids, size_t n_ids, const uint32_t* dbits, uint32_t* hit, hipStream_t stream);
// candidate list of each of points[0 .. nb): the walk of include/mse.h, scored against the point; list k to (cand_ids, cand_sc)[k * cap ..],
// its length to counts[k].  cap >= stride + stride^2.  table: scratch_bytes = delete_gather_table_bytes(stride, nb) (0: the walk's table
// fits the LDS).  stats[0] = longest list (max), stats[1] += lists longer than maxc
size_t delete_gather_table_bytes(int stride, size_t nb);
int launch_delete_gather(const uint16_t* base, size_t n, int d, const uint32_t* adj, const uint32_t* deg, int stride, const uint32_t* dbits,
                         const uint32_t* points, size_t nb, uint32_t* cand_ids, long long* cand_sc, size_t cap, uint32_t* counts, void* table,
                         int maxc, uint32_t* stats, uint32_t* err, hipStream_t stream);
// every member of D: empty list, has_url = 0, bit set in `deleted`
int launch_delete_finish(uint32_t* deg, uint8_t* has_url, uint32_t* deleted, const uint32_t* dbits, size_t n, hipStream_t stream);
// restore: bit cleared in `deleted`, has_url = 1
int launch_delete_restore(uint8_t* has_url, uint32_t* deleted, const uint32_t* ids, size_t n_ids, hipStream_t stream);

// ---- join.hip: the near-duplicate joins (include/mse.h mse_join_self / mse_join_cross) ------------------------
constexpr int JOIN_TILE = 128;   // rows per side of a Gram tile
struct JoinPair { uint32_t lo, hi; int64_t score; };
// One launch over a strip of the tile schedule: hi tiles h0 .. h0 + n_hi, tile t = (hi tile - h0) * span + x with lo tile = hi tile - x
// (x < span; tiles outside the triangle or the window band do not exist).  tile_base == null: the strip's FIRST launch -- every tile writes
// its nomination count to tile_count[t], reserves room at *cursor (zeroed by the caller) and stores its pairs if they end within cap;
// *tiles_run += tiles that did work.  tile_base != null (the exclusive prefix of tile_count): a WINDOW launch -- the nominations numbered
// win_lo .. win_lo + cap in tile order are stored at cand[number - win_lo]; tiles without one leave at once.
// The CROSS join (a second base of incoming rows in the hi role) has a rectangle instead: blockIdx.y walks the n_hi BASE tiles from h0,
// blockIdx.x the span INCOMING tiles from x0, tile t = y * span + x as above; every tile of the grid exists, window is 0 and `within`
// speaks for the base rows only
struct JoinStrip {
    uint32_t h0 = 0, n_hi = 0, span = 0;
    uint32_t x0 = 0;                                      // cross join: first incoming tile of the strip
    uint64_t window = 0;                                  // hi - lo <= window (0: no limit)
    const uint32_t* within = nullptr; size_t within_words = 0;   // bitmap words of an mse_filter (null: every row)
    uint32_t* tile_count = nullptr;
    const unsigned long long* tile_base = nullptr;
    unsigned long long win_lo = 0;
    unsigned long long* cursor = nullptr;
    unsigned long long* tiles_run = nullptr;
    uint2* cand = nullptr; unsigned long long cap = 0;     // nominated (lo, hi) pairs
};
size_t join_tile_lds_bytes();
// exact: every pair of the tile scored in reference order and nominated by score >= threshold; else the matrix-core tile, nominating by
// accumulator * 2^32 >= thr_lo (the caller's threshold - bound, rounded down to a double); d % 64 == 0 there.  incoming != null: the cross
// join's rectangle of m incoming rows (hi) by n base rows (lo)
int launch_join_tiles(bool exact, const uint16_t* base, size_t n, const uint16_t* incoming, size_t m, int d, const JoinStrip& sp, int64_t threshold,
                      double thr_lo, hipStream_t stream);
int launch_join_scan_tiles(const uint32_t* counts, size_t n_tiles, unsigned long long* out, hipStream_t stream);
// a lane quad per nominated pair: *kept += pairs with fast_dot >= threshold; those numbered below store_cap are appended to conf and counted
// into row_count[hi].  incoming != null: hi is a row of it (the cross join)
int launch_join_rescore(const uint16_t* base, const uint16_t* incoming, int d, const uint2* cand, size_t m, int64_t threshold, unsigned long long* kept, JoinPair* conf,
                        unsigned long long store_cap, uint32_t* row_count, int n_cu, hipStream_t stream);
// conf (count pairs, any order; row_count as the re-score left it, consumed) -> offsets [n + 1] over hi, and lo / hi / scores in canonical
// order: hi ascending, then lo ascending
int launch_join_csr(const JoinPair* conf, size_t count, size_t n, uint32_t* row_count, unsigned long long* offsets, uint32_t* lo, uint32_t* hi,
                    int64_t* scores, hipStream_t stream);
// one round of the keep-first rule: state 0 undecided / 1 kept / 2 dropped, in -> out; *undecided += rows still open
int launch_join_round(const unsigned long long* offsets, const uint32_t* lo, size_t n, const uint8_t* in, uint8_t* out, unsigned long long* undecided,
                      hipStream_t stream);
// rep, the dropped rows' bitmap (dup_words: whole 256-row tiles) and the group labels from the final state; has_member: n zeroed bytes
int launch_join_finish(const unsigned long long* offsets, const uint32_t* lo, size_t n, const uint8_t* state, uint32_t* rep, uint8_t* has_member,
                       uint32_t* dup_words, uint32_t* labels, hipStream_t stream);
// admission (mse_pairs_admit): state[j] = 2 for an incoming row with a cross pair, else 0 (1 when no rounds follow: `decide`);
// *undecided += rows left at 0
int launch_join_admit_init(const unsigned long long* cross_offsets, size_t m, bool decide, uint8_t* state, unsigned long long* undecided,
                           hipStream_t stream);
// from the final state: rep_base[j] = lowest base partner or ID_NONE; rep_incoming[j] = j (kept), the lowest kept earlier `among` neighbour
// (dropped by it), ID_NONE (dropped by the base); kept_words: the kept rows as bitmap words (whole 256-row tiles, zero past m).
// among_offsets null: no list among the incoming rows
int launch_join_admit_finish(const unsigned long long* cross_offsets, const uint32_t* cross_lo, const unsigned long long* among_offsets,
                             const uint32_t* among_lo, size_t m, const uint8_t* state, uint32_t* rep_base, uint32_t* rep_incoming,
                             uint32_t* kept_words, hipStream_t stream);
// out row j = in row ids[j], j < count, rows of row_bytes (a multiple of 16; both pointers 16-byte aligned)
int launch_join_select_rows(const void* in, size_t row_bytes, const uint32_t* ids, size_t count, void* out, int n_cu, hipStream_t stream);

// ---- scan_mfma.hip ---------------------------------------------------------------------------
// group_max[q_pad_index][g] layout: [n_groups][nq_pad] floats (group-major), nq_pad multiple of 32
int launch_scan_mfma(const uint16_t* base, size_t n_rows, int d, const uint16_t* queries_dev, int nq_pad,
                     void* packed_scratch, float* group_max, int n_cu, hipStream_t stream,
                     hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr, int gm_stride = 0 /* row stride of group_max; 0 = nq_pad */,
                     int n_pass = 1 /* passes in this launch: consecutive nq_pad-row query tiles, consecutive column ranges of group_max */,
                     const uint32_t* mask = nullptr, size_t mask_words = 0 /* filtered search: one bitmap word per 32-row group */,
                     int nq_rows = -1 /* query rows that exist at queries_dev, over all passes; the rest of the last pass is packed as
                                         zeros.  -1 = all n_pass x nq_pad */,
                     int group_rows = GROUP_ROWS /* base rows per written maximum: 32, or 64 (nq_pad 320 only) */);
                     // events bracket the scan kernel only
// One launch of the 320-query search kernel (64 rows per maximum, unmasked) over a SUBSET of the 256-row tiles: launch tile v of
// n_tiles is base tile v * mul + (v >> shift) + add.  tau == nullptr: the dense epilogue, into group_max [4 n_tiles][stride] indexed
// by the launch's own groups 4 v + rg.  tau != nullptr: a group maximum above tau[column] is appended to that column's list as
// (base group, maximum) -- counts[column] counts every survivor, stored or not; nothing dense is written.
struct ScanSparse {
    size_t n_tiles = 0;
    uint32_t mul = 1, shift = 63, add = 0;
    const float* tau = nullptr;
    uint32_t* counts = nullptr;
    uint32_t* ids = nullptr;
    float* keys = nullptr;
    uint32_t cap = 0;
};
// pack: re-tile the queries first (the first launch of a pass); the later launches of the pass reuse packed_scratch
int launch_scan_mfma_tiles(const uint16_t* base, size_t n_rows, int d, const uint16_t* queries_dev, int nq_rows, bool pack, void* packed_scratch,
                           const ScanSparse& sp, float* group_max, int n_cu, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end);
size_t mfma_packed_bytes(int d);
int mfma_query_tile(int d);  // most queries one pass handles at width d (320 or 256)
int mfma_pad(int nq, int d);   // padded query count of a pass of nq <= 256 queries: 128, 192 or 256
int mfma_group_rows(int nq_pad);   // rows per group maximum a search pass of that width asks for: 64 at 320 queries, else 32

}  // namespace mse
