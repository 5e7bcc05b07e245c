// Row groupings of the grouped ("collapse") search (include/mse.h mse_groups): one result per group.  Six device pieces (the fourth, the
// group step over the graph request path's unranked visited lists, its twin over the gathered blocks of a sharded search -- the grouped
// merge -- and the relabelling of a grouping cut to a shard's rows are described where they stand):
//   1. validation and count of a grouping: the largest non-NONE id, the NONE rows, the distinct ids (presence bitmap + popcount);
//   2. the order-preserving collapse of a ranked candidate list: one workgroup per query, an LDS open-addressing table keyed by group in
//      which every entry publishes its rank by atomic min; an entry whose own rank stands is its group's representative; the survivors
//      are compacted in list order (wave64 ballot, __popcll prefix, cross-wave offsets through LDS);
//   3. the dense path, for when no prefix of the ranking holds k groups: the best row of every group over ALL scores of a query by
//      integer atomics -- order-independent, so the result is bit-reproducible -- and every other grouped row demoted to the lowest key,
//      so that the ordinary tournament over level 0 ranks representatives first.
// Same-address contention: a group of thousands of rows puts thousands of atomics on one address.  Same-address float atomic ADDS are
// measured an order of magnitude slower than spread ones on this chip; integer max / min at one address are NOT measured.  Frames of
// one video are consecutive rows, so each wave first reduces over runs of adjacent lanes with equal group, and a run issues its atomic
// only if a plain read of the table does not already hold as much (max and min are monotone, so a stale read is harmless).
#include "common.h"
#include "kernels.h"
#include <algorithm>
#include <cfloat>

namespace mse {
namespace {

constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;
constexpr int COLLAPSE_THREADS = 256;
constexpr int COLLAPSE_MAX = 2048;    // longest list one workgroup collapses
constexpr int COLLAPSE_TABLE = 4096;  // table slots: twice the longest list, so a probe always ends at a free slot
constexpr int COLLAPSE_PER_THREAD = COLLAPSE_MAX / COLLAPSE_THREADS;

// ---- 1. validation and count -----------------------------------------------------------------------------------------------------------
// stats[0] = max over non-NONE ids of id + 1 (0: none), stats[1] += NONE rows; the bit of every id below n_rows is set in `present`
// (zeroed, (n_rows + 31) / 32 words).  An id at or past n_rows sets no bit: it is reported through stats[0] and nothing is made.
__global__ __launch_bounds__(256) void groups_validate_kernel(const uint32_t* __restrict__ group_of, size_t n_rows, uint32_t* __restrict__ present,
                                                             unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_max[4], s_none[4];
    unsigned long long top = 0, none = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t g = group_of[i];
        if (g == GROUP_NONE) { none++; continue; }
        if ((unsigned long long)g + 1 > top) top = (unsigned long long)g + 1;
        if (g < n_rows) atomicOr(&present[g >> 5], 1u << (g & 31));
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(top, off);
        top = o > top ? o : top;
        none += __shfl_xor(none, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_max[wave] = top; s_none[wave] = none; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) { top = s_max[w] > top ? s_max[w] : top; none += s_none[w]; }
        if (top) atomicMax(&stats[0], top);
        if (none) atomicAdd(&stats[1], none);
    }
}

// stats[2] += set bits of `present`
__global__ __launch_bounds__(256) void groups_popcount_kernel(const uint32_t* __restrict__ present, size_t n_words, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_sum[4];
    unsigned long long c = 0;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (size_t)gridDim.x * blockDim.x) c += (unsigned)__popc(present[w]);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        c = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (c) atomicAdd(&stats[2], c);
    }
}

// ---- 2. collapse of a ranked list ------------------------------------------------------------------------------------------------------
// One workgroup per query.  ids [nq][ids_stride], best first, ID_NONE padding at the tail only, n_list <= COLLAPSE_MAX entries read.
// kept_pos [nq][k]: positions of the first k representatives (ID_NONE padded); n_reps [nq]: representatives in the whole list.
__global__ __launch_bounds__(COLLAPSE_THREADS) void collapse_kernel(const uint32_t* __restrict__ ids, size_t ids_stride, int n_list,
                                                                    const uint32_t* __restrict__ group_of, size_t g_len, int k,
                                                                    uint32_t* __restrict__ kept_pos, uint32_t* __restrict__ n_reps) {
    __shared__ uint32_t t_key[COLLAPSE_TABLE];    // group id, GROUP_NONE = free (a NONE row is never inserted)
    __shared__ uint32_t t_rank[COLLAPSE_TABLE];   // lowest list position seen under that key
    __shared__ uint32_t wave_tot[COLLAPSE_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t q = blockIdx.x;
    for (int i = t; i < COLLAPSE_TABLE; i += COLLAPSE_THREADS) { t_key[i] = GROUP_NONE; t_rank[i] = 0xFFFFFFFFu; }
    __syncthreads();
    // entry c * 256 + t belongs to this thread: consecutive lanes hold consecutive list positions, which the compaction relies on
    uint32_t slot[COLLAPSE_PER_THREAD];   // table slot of the entry; TABLE = a representative by rule (NONE / past the grouping); TABLE + 1 = no entry
#pragma unroll
    for (int c = 0; c < COLLAPSE_PER_THREAD; c++) {
        const int i = c * COLLAPSE_THREADS + t;
        slot[c] = COLLAPSE_TABLE + 1;
        if (i >= n_list) continue;
        const uint32_t id = ids[q * ids_stride + i];
        if (id == ID_NONE) continue;
        const uint32_t g = id < g_len ? group_of[id] : GROUP_NONE;
        if (g == GROUP_NONE) { slot[c] = COLLAPSE_TABLE; continue; }
        uint32_t h = (g * 2654435761u) >> 20;   // 12 bits
        for (;;) {   // at most n_list <= TABLE / 2 keys are ever inserted: a free slot or the key itself is always found
            const uint32_t prev = atomicCAS(&t_key[h], GROUP_NONE, g);
            if (prev == GROUP_NONE || prev == g) break;
            h = (h + 1) & (COLLAPSE_TABLE - 1);
        }
        atomicMin(&t_rank[h], (uint32_t)i);
        slot[c] = h;
    }
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int c = 0; c < COLLAPSE_PER_THREAD; c++) {
        if (c * COLLAPSE_THREADS >= n_list) break;   // uniform
        const int i = c * COLLAPSE_THREADS + t;
        const bool rep = slot[c] == COLLAPSE_TABLE || (slot[c] < COLLAPSE_TABLE && t_rank[slot[c]] == (uint32_t)i);
        const unsigned long long m = __ballot(rep);
        if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        uint32_t total = 0;
        for (int w = 0; w < COLLAPSE_THREADS / 64; w++) {
            if (w < wave) pos += wave_tot[w];
            total += wave_tot[w];
        }
        if (rep && pos < (uint32_t)k) kept_pos[q * k + pos] = (uint32_t)i;
        base += total;
        __syncthreads();
    }
    for (uint32_t j = base + t; j < (uint32_t)k; j += COLLAPSE_THREADS) kept_pos[q * k + j] = ID_NONE;
    if (t == 0) n_reps[q] = base;
}

// the entries at kept_pos, with their payload (key_bytes 8: i64 scores, padding INT64_MIN; 4: f32 keys, padding -FLT_MAX), into row
// dst_rows[q] (null: q) of the outputs -- for the queries with take[q] != 0 (null: all)
__global__ void collapse_gather_kernel(const uint32_t* __restrict__ kept_pos, int k, const uint32_t* __restrict__ ids, size_t ids_stride,
                                       const void* __restrict__ keys, size_t keys_stride, int key_bytes, int nq, uint64_t id_offset,
                                       const uint32_t* __restrict__ dst_rows, const uint8_t* __restrict__ take, void* __restrict__ out_keys,
                                       uint32_t* __restrict__ out_ids, size_t out_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nq * k) return;
    const size_t q = i / k, j = i % k;
    if (take && !take[q]) return;
    const size_t row = dst_rows ? dst_rows[q] : q;
    const uint32_t p = kept_pos[i];
    uint32_t id = ID_NONE;
    if (p != ID_NONE) id = ids[q * ids_stride + p];
    out_ids[row * out_stride + j] = id == ID_NONE ? ID_NONE : (uint32_t)(id + id_offset);
    if (key_bytes == 8)
        reinterpret_cast<int64_t*>(out_keys)[row * out_stride + j] = id == ID_NONE ? INT64_MIN : reinterpret_cast<const int64_t*>(keys)[q * keys_stride + p];
    else
        reinterpret_cast<float*>(out_keys)[row * out_stride + j] = id == ID_NONE ? -FLT_MAX : reinterpret_cast<const float*>(keys)[q * keys_stride + p];
}

// ---- 3. dense path ---------------------------------------------------------------------------------------------------------------------
// Level 0 of a query holds one key per list position p < n (row = list[p], or p without a list; ascending either way).
// best [nq][g_len] u64, zeroed:  I64: max over the group's rows of the order-preserving key; F32: max of (key32 << 32) | ~row, which
// decides score and id at once.  best_id [nq][g_len] u32, all ones (I64 only): the lowest row among those that hold the maximum.
template <bool F32>
__device__ __forceinline__ unsigned long long dense_value(const void* scores, size_t at, uint32_t row) {
    if (F32) return ((unsigned long long)sortable_f32_bits(reinterpret_cast<const uint32_t*>(scores)[at]) << 32) | (uint32_t)~row;
    return sortable_i64(reinterpret_cast<const int64_t*>(scores)[at]);
}

// lane's run: the adjacent lanes of the wave with the same group.  *start = first lane of the run, *last = this lane ends it
__device__ __forceinline__ void wave_run(uint32_t g, int lane, int* start, bool* last) {
    const uint32_t prev = __shfl_up(g, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != g);
    *start = 63 - __clzll(heads & ((2ull << lane) - 1ull));   // (2 << 63 wraps to 0, minus 1 = all ones: lane 63 sees every head)
    *last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
}

template <bool F32>
__global__ __launch_bounds__(256) void dense_max_kernel(const void* __restrict__ scores, size_t stride, size_t n, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ group_of, size_t g_len,
                                                       unsigned long long* __restrict__ best) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // whole waves run to the end: the shuffles need every lane
    const size_t q = blockIdx.y;
    const int lane = threadIdx.x & 63;
    uint32_t g = GROUP_NONE;
    unsigned long long v = 0;
    if (p < n) {
        const uint32_t row = list ? list[p] : (uint32_t)p;
        if (row < g_len) g = group_of[row];
        if (g != GROUP_NONE) v = dense_value<F32>(scores, q * stride + p, row);
    }
    int start; bool last;
    wave_run(g, lane, &start, &last);
    for (int off = 1; off < 64; off <<= 1) {   // segmented inclusive max scan: the run's last lane ends with the run's maximum
        const unsigned long long o = __shfl_up(v, off);
        if (lane - off >= start && o > v) v = o;
    }
    // the table only grows: a value read now that is already at least v makes the atomic pointless (a stale, lower read merely costs
    // one).  With thousands of rows on one address this leaves the first few waves' atomics and a cached load for the rest.
    if (last && g != GROUP_NONE) {
        unsigned long long* at = &best[q * g_len + g];
        if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(at, v);
    }
}

__global__ __launch_bounds__(256) void dense_min_id_kernel(const int64_t* __restrict__ scores, size_t stride, size_t n, const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ group_of, size_t g_len,
                                                          const unsigned long long* __restrict__ best, uint32_t* __restrict__ best_id) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t q = blockIdx.y;
    const int lane = threadIdx.x & 63;
    uint32_t g = GROUP_NONE, row = 0;
    bool holds = false;
    if (p < n) {
        row = list ? list[p] : (uint32_t)p;
        if (row < g_len) g = group_of[row];
        if (g != GROUP_NONE) holds = sortable_i64(scores[q * stride + p]) == best[q * g_len + g];
    }
    int start; bool last;
    wave_run(g, lane, &start, &last);
    // rows ascend with the lane: of a run only the first lane that holds the maximum can be the lowest id
    const unsigned long long m = __ballot(holds);
    const unsigned long long before = m & ((1ull << lane) - 1ull) & ~((1ull << start) - 1ull);
    if (holds && before == 0) {   // (as above: the id only falls)
        uint32_t* at = &best_id[q * g_len + g];
        if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row) atomicMin(at, row);
    }
}

// every grouped row that is not its group's representative drops to the lowest key: INT64_MIN, or the all-ones f32 pattern (a NaN no dot
// product produces, below every other key in the sortable order).  I64: n_sat[q] counts the representatives and ungrouped rows whose OWN
// score is INT64_MIN (saturated): they tie with the demoted rows, and dense_complete_kernel finishes a short list from them.
template <bool F32>
__global__ __launch_bounds__(256) void dense_demote_kernel(void* __restrict__ scores, size_t stride, size_t n, const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ group_of, size_t g_len,
                                                          const unsigned long long* __restrict__ best, const uint32_t* __restrict__ best_id,
                                                          uint32_t* __restrict__ n_sat) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t q = blockIdx.y;
    if (p >= n) return;
    const uint32_t row = list ? list[p] : (uint32_t)p;
    const uint32_t g = row < g_len ? group_of[row] : GROUP_NONE;
    const size_t at = q * stride + p;
    if (F32) {
        if (g != GROUP_NONE && dense_value<true>(scores, at, row) != best[q * g_len + g]) reinterpret_cast<uint32_t*>(scores)[at] = 0xFFFFFFFFu;
    } else {
        int64_t* sc = reinterpret_cast<int64_t*>(scores);
        if (g != GROUP_NONE && best_id[q * g_len + g] != row) sc[at] = INT64_MIN;
        else if (sc[at] == INT64_MIN) atomicAdd(&n_sat[q], 1u);
    }
}

// I64, one workgroup per query, for the degenerate case only: a list with fewer than k representatives although saturated
// representatives exist.  The representatives above INT64_MIN are all on the list already (they outrank every demoted row, and there are
// fewer than k of them); behind them go the saturated ones in id order, found by one ordered walk over level 0.
__global__ __launch_bounds__(256) void dense_complete_kernel(const int64_t* __restrict__ scores, size_t stride, size_t n, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ group_of, size_t g_len, const uint32_t* __restrict__ best_id,
                                                            const uint32_t* __restrict__ n_sat, const uint32_t* __restrict__ kept_pos,
                                                            const uint32_t* __restrict__ n_reps, const int64_t* __restrict__ sel_keys, int k,
                                                            uint64_t id_offset, const uint32_t* __restrict__ dst_rows, int64_t* __restrict__ out_scores,
                                                            uint32_t* __restrict__ out_ids, size_t out_stride) {
    __shared__ uint32_t s_above, wave_tot[4];
    const size_t q = blockIdx.x;
    const uint32_t reps = n_reps[q];
    if (reps >= (uint32_t)k || n_sat[q] == 0) return;   // uniform
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_above = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t j = t; j < reps; j += 256) mine += sel_keys[q * k + kept_pos[q * k + j]] != INT64_MIN;
    if (mine) atomicAdd(&s_above, mine);
    __syncthreads();
    uint32_t base = s_above;
    const size_t dst = dst_rows ? dst_rows[q] : q;
    for (size_t p0 = 0; p0 < n && base < (uint32_t)k; p0 += 256) {   // uniform: base is the same in every thread
        const size_t p = p0 + t;
        bool is = false;
        uint32_t row = 0;
        if (p < n && scores[q * stride + p] == INT64_MIN) {
            row = list ? list[p] : (uint32_t)p;
            const uint32_t g = row < g_len ? group_of[row] : GROUP_NONE;
            is = g == GROUP_NONE || best_id[q * g_len + g] == row;
        }
        const unsigned long long m = __ballot(is);
        if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) pos += wave_tot[w];
            total += wave_tot[w];
        }
        if (is && pos < (uint32_t)k) {
            out_scores[dst * out_stride + pos] = INT64_MIN;
            out_ids[dst * out_stride + pos] = (uint32_t)(row + id_offset);
        }
        base += total;
        __syncthreads();
    }
}

// ---- 4. group step over an UNRANKED visited list (graph request path, beam_search.hip read_back_fused) ---------------------------------
// One workgroup per query over vis_ids / vis_scores [nq][cap], n = min(n_visited[q], cap) records in visit order, holes (ID_NONE,
// INT64_MIN) where the de-duplication removed a record.  Of every group that has a live record the best one by (score desc, id asc)
// stays; every other record of the group becomes a hole in place, exactly as dedup_filter_batch_kernel leaves one, so the selection that
// follows needs no change.  Records of group NONE or past the grouping, holes, and entries at or past n are not touched.
// Open-addressing table keyed by group (collapse_kernel's multiplicative hash, linear probing), 16 bytes per slot -- best key u64 | group
// u32 | id u32, three arrays -- of which a query clears and uses only the power of two of at least 2 n slots (64 at least): at most n keys
// are ever inserted, so a probe always ends at the key or at a free slot.  A slot is claimed by compare-and-swap; the group's best score
// is an atomic max of the order-preserving key; after a barrier, an atomic min of the id among the records that hold the maximum; after
// a second barrier a record stays only if its slot holds its id.  Integer max and min do not depend on arrival order: bit-reproducible.
// GLOBAL = false: the table in dynamic LDS (cap <= 4096).  true: in global memory, slots_cap slots per query of the launch; its words
// are read and cleared through agent-scope atomics, so that no wave reads a stale cached line after another wave's atomic.
constexpr int VG_THREADS = 256;
constexpr size_t VG_LDS_CAP = 4096;                       // longest list whose table (8192 slots, 128 KiB) fits dynamic LDS
constexpr size_t VG_TABLE_BUDGET = (size_t)32 << 20;      // global tables of one launch (a query chunk), bytes

template <bool GLOBAL, typename T>
__device__ __forceinline__ T vg_load(const T* p) {
    if (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool GLOBAL, typename T>
__device__ __forceinline__ void vg_store(T* p, T v) {
    if (GLOBAL) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// Where the records of one query's list live.  Flat: one contiguous list, the request path's visited list.  Blocks: the gathered
// packed blocks of a sharded search (shard_group.hip merge_packed's addressing) -- record i is record i % k_in of shard i / k_in, a
// shard's ids / scores of the query id_stride / sc_stride elements after the previous shard's.
struct VgFlat {
    uint32_t* ids; long long* scores;
    __device__ __forceinline__ uint32_t* id_at(uint32_t i) const { return ids + i; }
    __device__ __forceinline__ long long* score_at(uint32_t i) const { return scores + i; }
};
struct VgBlocks {
    uint32_t* ids; long long* scores; uint32_t k_in; size_t id_stride, sc_stride;
    __device__ __forceinline__ uint32_t* id_at(uint32_t i) const { return ids + (size_t)(i / k_in) * id_stride + i % k_in; }
    __device__ __forceinline__ long long* score_at(uint32_t i) const { return scores + (size_t)(i / k_in) * sc_stride + i % k_in; }
};

template <bool GLOBAL, typename Rec>
__device__ __forceinline__ void visited_group_body(const Rec rec, uint32_t n, const uint32_t* __restrict__ group_of, size_t g_len, uint32_t bits,
                                                   unsigned long long* t_best, uint32_t* t_key, uint32_t* t_id) {
    const uint32_t t = threadIdx.x, slots = 1u << bits, mask = slots - 1u;
    for (uint32_t i = t; i < slots; i += VG_THREADS) {
        vg_store<GLOBAL>(&t_best[i], 0ull);
        vg_store<GLOBAL>(&t_key[i], GROUP_NONE);
        vg_store<GLOBAL>(&t_id[i], 0xFFFFFFFFu);
    }
    __syncthreads();
    auto group = [&](uint32_t id) { return id != ID_NONE && id < g_len ? group_of[id] : GROUP_NONE; };
    for (uint32_t i = t; i < n; i += VG_THREADS) {   // claim the group's slot, publish the score
        const uint32_t g = group(*rec.id_at(i));
        if (g == GROUP_NONE) continue;
        uint32_t h = (g * 2654435761u) >> (32 - bits);
        for (;;) {
            const uint32_t prev = atomicCAS(&t_key[h], GROUP_NONE, g);
            if (prev == GROUP_NONE || prev == g) break;
            h = (h + 1) & mask;
        }
        const unsigned long long v = sortable_i64(*rec.score_at(i));
        if (vg_load<GLOBAL>(&t_best[h]) < v) atomicMax(&t_best[h], v);   // (the slot only grows: a stale, lower read merely costs the atomic)
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += VG_THREADS) {   // among the records that hold the maximum, the lowest id
        const uint32_t id = *rec.id_at(i), g = group(id);
        if (g == GROUP_NONE) continue;
        uint32_t h = (g * 2654435761u) >> (32 - bits);
        while (vg_load<GLOBAL>(&t_key[h]) != g) h = (h + 1) & mask;   // (entered above)
        if (sortable_i64(*rec.score_at(i)) == vg_load<GLOBAL>(&t_best[h]) && vg_load<GLOBAL>(&t_id[h]) > id) atomicMin(&t_id[h], id);
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += VG_THREADS) {   // everything else of the group leaves the list
        const uint32_t id = *rec.id_at(i), g = group(id);
        if (g == GROUP_NONE) continue;
        uint32_t h = (g * 2654435761u) >> (32 - bits);
        while (vg_load<GLOBAL>(&t_key[h]) != g) h = (h + 1) & mask;
        if (vg_load<GLOBAL>(&t_id[h]) != id) { *rec.id_at(i) = ID_NONE; *rec.score_at(i) = (long long)INT64_MIN; }
    }
}

// the query's table: best keys | groups | ids of the slots in use, packed at its front (two call sites, so that each inlined copy of the
// body knows its address space: LDS atomics stay ds_ instructions)
template <bool GLOBAL, typename Rec>
__device__ __forceinline__ void visited_group_run(const Rec rec, uint32_t n, const uint32_t* __restrict__ group_of, size_t g_len, char* smem,
                                                  unsigned long long* table, size_t q, uint32_t slots_cap) {
    uint32_t bits = 6;
    while ((1u << bits) < 2u * n) bits++;   // <= slots_cap: n <= cap
    if constexpr (GLOBAL) {
        char* tab = reinterpret_cast<char*>(table) + q * (size_t)slots_cap * 16;
        visited_group_body<true>(rec, n, group_of, g_len, bits, reinterpret_cast<unsigned long long*>(tab),
                                 reinterpret_cast<uint32_t*>(tab + ((size_t)8 << bits)), reinterpret_cast<uint32_t*>(tab + ((size_t)12 << bits)));
    } else {
        visited_group_body<false>(rec, n, group_of, g_len, bits, reinterpret_cast<unsigned long long*>(smem),
                                  reinterpret_cast<uint32_t*>(smem + ((size_t)8 << bits)), reinterpret_cast<uint32_t*>(smem + ((size_t)12 << bits)));
    }
}

template <bool GLOBAL>
__global__ __launch_bounds__(VG_THREADS) void visited_group_kernel(uint32_t* __restrict__ vis_ids, long long* __restrict__ vis_scores, size_t cap,
                                                                   const uint32_t* __restrict__ n_visited, const uint32_t* __restrict__ group_of,
                                                                   size_t g_len, unsigned long long* __restrict__ table, uint32_t slots_cap) {
    extern __shared__ __attribute__((aligned(16))) char vg_smem[];
    const size_t q = blockIdx.x;
    const uint32_t n = (uint32_t)min((size_t)n_visited[q], cap);
    visited_group_run<GLOBAL>(VgFlat{vis_ids + q * cap, vis_scores + q * cap}, n, group_of, g_len, vg_smem, table, q, slots_cap);
}

// ---- 5. the grouped merge of a sharded search (shard_group.hip) -------------------------------------------------------------------------
// The same step over the gathered packed blocks, in place: n_shards blocks of {[nq][k_in] i64 scores, [nq][k_in] u32 GLOBAL ids},
// block_bytes apart; query q0 + blockIdx.x (a launch takes a chunk of queries when the table is in global memory: its row of the table
// is blockIdx.x).  group_of is the GLOBAL grouping.  Every record of the n_shards * k_in of a query is looked at: holes and padding
// (ID_NONE) anywhere are skipped by the body.
template <bool GLOBAL>
__global__ __launch_bounds__(VG_THREADS) void merge_group_kernel(char* __restrict__ blocks, size_t block_bytes, uint32_t n_shards, size_t nq, size_t q0,
                                                                 uint32_t k_in, const uint32_t* __restrict__ group_of, size_t g_len,
                                                                 unsigned long long* __restrict__ table, uint32_t slots_cap) {
    extern __shared__ __attribute__((aligned(16))) char vg_smem[];
    const size_t q = q0 + blockIdx.x;
    const VgBlocks rec{reinterpret_cast<uint32_t*>(blocks + nq * k_in * 8) + q * k_in, reinterpret_cast<long long*>(blocks) + q * k_in, k_in,
                       block_bytes / 4, block_bytes / 8};
    visited_group_run<GLOBAL>(rec, n_shards * k_in, group_of, g_len, vg_smem, table, blockIdx.x, slots_cap);
}

// ---- 6. a grouping cut to a row range and relabelled (mse_groups_slice) -----------------------------------------------------------------
// labels [m]: the source's labels of the slice's rows (each below src_len, or NONE); table [src_len] u32, uninitialised.  Three launches
// on one stream: the entries the slice touches are set to all ones, every row publishes its local id under its label by atomic min, and a
// row's new label is what stands under its old one -- the local id of the first row of its group inside the slice.  Order-independent.
__global__ __launch_bounds__(256) void groups_slice_clear_kernel(const uint32_t* __restrict__ labels, size_t m, uint32_t* __restrict__ table) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t g = labels[i];
    if (g != GROUP_NONE) table[g] = 0xFFFFFFFFu;
}
__global__ __launch_bounds__(256) void groups_slice_min_kernel(const uint32_t* __restrict__ labels, size_t m, uint32_t* __restrict__ table) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t g = labels[i];
    if (g == GROUP_NONE) return;   // (the entry only falls: a stale, higher read merely costs the atomic)
    if (__hip_atomic_load(&table[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i) atomicMin(&table[g], (uint32_t)i);
}
__global__ __launch_bounds__(256) void groups_slice_lookup_kernel(const uint32_t* __restrict__ labels, size_t m, const uint32_t* __restrict__ table,
                                                                 uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t g = labels[i];
    out[i] = g == GROUP_NONE ? GROUP_NONE : table[g];
}

// table slots a list of up to `cap` records may need: the power of two of at least 2 cap (64 at least)
size_t visited_group_slots(size_t cap) {
    size_t slots = 64;
    while (slots < 2 * cap) slots *= 2;
    return slots;
}

}  // namespace

// queries of one launch: all of them with the table in LDS, else what the fixed table budget holds (the way launch_dedup_batch chunks)
static size_t visited_group_chunk_queries(size_t nq, size_t cap) {
    if (cap <= VG_LDS_CAP) return nq;
    return std::max<size_t>(1, std::min(nq, VG_TABLE_BUDGET / (visited_group_slots(cap) * 16)));
}

size_t visited_group_scratch_bytes(size_t nq, size_t cap) {
    return cap <= VG_LDS_CAP ? 0 : visited_group_chunk_queries(nq, cap) * visited_group_slots(cap) * 16;
}

int launch_visited_group(uint32_t* vis_ids, long long* vis_scores, size_t cap, const uint32_t* n_visited, size_t nq, const uint32_t* group_of,
                         size_t g_len, void* table, hipStream_t stream) {
    if (nq == 0 || cap == 0) return 0;
    if (cap > ((size_t)1 << 30)) return fail("visited_group: list too long");
    const size_t slots = visited_group_slots(cap);
    if (cap <= VG_LDS_CAP) {
        MSE_DYN_LDS(visited_group_kernel<false>, slots * 16);
        hipLaunchKernelGGL(visited_group_kernel<false>, dim3((unsigned)nq), dim3(VG_THREADS), slots * 16, stream, vis_ids, vis_scores, cap, n_visited,
                           group_of, g_len, (unsigned long long*)nullptr, (uint32_t)slots);
        MSE_HIP_TRY(hipGetLastError());
        return 0;
    }
    if (!table) return fail("visited_group: no table");
    const size_t chunk = visited_group_chunk_queries(nq, cap);
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {   // chunks run one after the other on the stream: they share the table
        const size_t m = std::min(chunk, nq - q0);
        hipLaunchKernelGGL(visited_group_kernel<true>, dim3((unsigned)m), dim3(VG_THREADS), 0, stream, vis_ids + q0 * cap, vis_scores + q0 * cap, cap,
                           n_visited + q0, group_of, g_len, static_cast<unsigned long long*>(table), (uint32_t)slots);
        MSE_HIP_TRY(hipGetLastError());
    }
    return 0;
}

size_t merge_group_scratch_bytes(size_t nq, size_t n_records) { return visited_group_scratch_bytes(nq, n_records); }

int launch_merge_group(void* blocks, size_t block_bytes, size_t n_shards, size_t nq, size_t k_in, const uint32_t* group_of, size_t g_len, void* table,
                       hipStream_t stream) {
    const size_t n = n_shards * k_in;
    if (nq == 0 || n == 0) return 0;
    if (n > ((size_t)1 << 30) || k_in > 0xFFFFFFFFull) return fail("merge_group: too many records per query");
    if (block_bytes % 8 || block_bytes < nq * k_in * 12) return fail("merge_group: bad block stride");
    const size_t slots = visited_group_slots(n);
    if (n <= VG_LDS_CAP) {
        MSE_DYN_LDS(merge_group_kernel<false>, slots * 16);
        hipLaunchKernelGGL(merge_group_kernel<false>, dim3((unsigned)nq), dim3(VG_THREADS), slots * 16, stream, static_cast<char*>(blocks), block_bytes,
                           (uint32_t)n_shards, nq, (size_t)0, (uint32_t)k_in, group_of, g_len, (unsigned long long*)nullptr, (uint32_t)slots);
        MSE_HIP_TRY(hipGetLastError());
        return 0;
    }
    if (!table) return fail("merge_group: no table");
    const size_t chunk = visited_group_chunk_queries(nq, n);
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {   // chunks run one after the other on the stream: they share the table
        const size_t m = std::min(chunk, nq - q0);
        hipLaunchKernelGGL(merge_group_kernel<true>, dim3((unsigned)m), dim3(VG_THREADS), 0, stream, static_cast<char*>(blocks), block_bytes,
                           (uint32_t)n_shards, nq, q0, (uint32_t)k_in, group_of, g_len, static_cast<unsigned long long*>(table), (uint32_t)slots);
        MSE_HIP_TRY(hipGetLastError());
    }
    return 0;
}

int launch_groups_slice(const uint32_t* labels, size_t m, uint32_t* table, uint32_t* out, hipStream_t stream) {
    if (m == 0) return 0;
    const dim3 grid((unsigned)((m + 255) / 256)), block(256);
    hipLaunchKernelGGL(groups_slice_clear_kernel, grid, block, 0, stream, labels, m, table);
    MSE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(groups_slice_min_kernel, grid, block, 0, stream, labels, m, table);
    MSE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(groups_slice_lookup_kernel, grid, block, 0, stream, labels, m, (const uint32_t*)table, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_groups_validate(const uint32_t* group_of, size_t n_rows, uint32_t* present, unsigned long long* stats, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const unsigned blocks = (unsigned)std::min<size_t>((n_rows + 255) / 256, 4096);
    hipLaunchKernelGGL(groups_validate_kernel, dim3(blocks), dim3(256), 0, stream, group_of, n_rows, present, stats);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_groups_popcount(const uint32_t* present, size_t n_words, unsigned long long* stats, hipStream_t stream) {
    if (n_words == 0) return 0;
    const unsigned blocks = (unsigned)std::min<size_t>((n_words + 255) / 256, 4096);
    hipLaunchKernelGGL(groups_popcount_kernel, dim3(blocks), dim3(256), 0, stream, present, n_words, stats);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_collapse(const uint32_t* ids, size_t ids_stride, size_t n_list, const uint32_t* group_of, size_t g_len, int k, int nq,
                    uint32_t* kept_pos, uint32_t* n_reps, hipStream_t stream) {
    if (nq <= 0) return 0;
    if (n_list == 0 || n_list > (size_t)COLLAPSE_MAX) return fail("collapse: 1.." + std::to_string(COLLAPSE_MAX) + " entries per list");
    if (k <= 0 || n_list > ids_stride) return fail("collapse: bad k or stride");
    hipLaunchKernelGGL(collapse_kernel, dim3((unsigned)nq), dim3(COLLAPSE_THREADS), 0, stream, ids, ids_stride, (int)n_list, group_of, g_len, k,
                       kept_pos, n_reps);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_collapse_gather(const uint32_t* kept_pos, int k, const uint32_t* ids, size_t ids_stride, const void* keys, size_t keys_stride,
                           int key_bytes, int nq, uint64_t id_offset, const uint32_t* dst_rows, const uint8_t* take, void* out_keys,
                           uint32_t* out_ids, size_t out_stride, hipStream_t stream) {
    if (nq <= 0 || k <= 0) return 0;
    if (key_bytes != 4 && key_bytes != 8) return fail("collapse_gather: payload of 4 or 8 bytes");
    const size_t total = (size_t)nq * k;
    hipLaunchKernelGGL(collapse_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, kept_pos, k, ids, ids_stride, keys,
                       keys_stride, key_bytes, nq, id_offset, dst_rows, take, out_keys, out_ids, out_stride);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_dense_group_best(bool f32, void* scores, size_t stride, size_t n, const uint32_t* list, const uint32_t* group_of, size_t g_len, int nq,
                            unsigned long long* best, uint32_t* best_id, uint32_t* n_sat, hipStream_t stream, hipEvent_t ev_mid) {
    if (nq <= 0 || n == 0 || g_len == 0) return 0;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nq), block(256);
    MSE_HIP_TRY(hipMemsetAsync(best, 0, (size_t)nq * g_len * 8, stream));
    if (f32) {
        hipLaunchKernelGGL(dense_max_kernel<true>, grid, block, 0, stream, (const void*)scores, stride, n, list, group_of, g_len, best);
        MSE_HIP_TRY(hipGetLastError());
        if (ev_mid) MSE_HIP_TRY(hipEventRecord(ev_mid, stream));
        hipLaunchKernelGGL(dense_demote_kernel<true>, grid, block, 0, stream, scores, stride, n, list, group_of, g_len,
                           (const unsigned long long*)best, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    } else {
        MSE_HIP_TRY(hipMemsetAsync(best_id, 0xFF, (size_t)nq * g_len * 4, stream));
        MSE_HIP_TRY(hipMemsetAsync(n_sat, 0, (size_t)nq * 4, stream));
        hipLaunchKernelGGL(dense_max_kernel<false>, grid, block, 0, stream, (const void*)scores, stride, n, list, group_of, g_len, best);
        MSE_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(dense_min_id_kernel, grid, block, 0, stream, (const int64_t*)scores, stride, n, list, group_of, g_len,
                           (const unsigned long long*)best, best_id);
        MSE_HIP_TRY(hipGetLastError());
        if (ev_mid) MSE_HIP_TRY(hipEventRecord(ev_mid, stream));
        hipLaunchKernelGGL(dense_demote_kernel<false>, grid, block, 0, stream, scores, stride, n, list, group_of, g_len,
                           (const unsigned long long*)best, (const uint32_t*)best_id, n_sat);
    }
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_dense_complete(const int64_t* scores, size_t stride, size_t n, const uint32_t* list, const uint32_t* group_of, size_t g_len,
                          const uint32_t* best_id, const uint32_t* n_sat, const uint32_t* kept_pos, const uint32_t* n_reps, const int64_t* sel_keys,
                          int k, int nq, uint64_t id_offset, const uint32_t* dst_rows, int64_t* out_scores, uint32_t* out_ids, size_t out_stride,
                          hipStream_t stream) {
    if (nq <= 0 || n == 0 || g_len == 0) return 0;
    hipLaunchKernelGGL(dense_complete_kernel, dim3((unsigned)nq), dim3(256), 0, stream, scores, stride, n, list, group_of, g_len, best_id, n_sat,
                       kept_pos, n_reps, sel_keys, k, id_offset, dst_rows, out_scores, out_ids, out_stride);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mse
