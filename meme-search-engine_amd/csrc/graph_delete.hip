// Delete consolidation on the device: rows leave a live graph index and the lists that pointed at them are repaired (FreshDiskANN's
// delete consolidation, stated deterministically in include/mse.h "delete rows and repair the graph").
//
// D = the delete set (a bitmap, one bit per node), N(x) = the list of x when the call started.  Four steps:
//   mark     delete_mark_kernel      one wave per list tests its entries against D; the affected nodes -- not in D, listing a member of D --
//                                    come out as a bitmap (a workgroup owns one 32-node word: no atomics), which the filter compaction
//                                    (filter.hip) turns into an ascending id list.  The same pass validates every edge.
//   gather   delete_gather_kernel    one workgroup per affected node p: the walk over N(p), a deleted entry v replaced by N(v); members of
//                                    D and p itself dropped; duplicates dropped through an open-addressing table keyed by id that keeps the
//                                    SMALLEST walk position, so "first occurrence" survives the parallel insert; survivors compacted in
//                                    walk order by a prefix sum over a position bitmap; each scored against row p by the exact quad-lane
//                                    dot (exact_dot.h: six 16-byte pieces per lane in flight); (id, score) to the candidate slab in HBM.
//   prune    prune_kernel / apply_lists_kernel of graph_build.hip, unchanged: stable sort, cut to maxc, alpha walk, saturate.
//   finish   delete_finish_kernel    members of D: empty list, has_url = 0, bit set in the graph's deleted map.
// Every candidate list reads start-of-call lists only (a live list is written by its own node's work, the deleted lists are emptied
// last), so the result does not depend on the batching.  The candidate slab and the tables are sized by the batch, not the graph.
#include "../../include/mse.h"
#include "exact_dot.h"
#include "runtime.h"
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

using namespace mse;

namespace {

constexpr int GD_THREADS = 256;
constexpr int GD_SMAX = 128;                                   // widest list a graph may have here
constexpr int GD_FLAGW = (GD_SMAX * (GD_SMAX + 1) + 31) / 32 + 4;   // words of the walk-position bitmap (520)
constexpr int GD_WPT = (GD_FLAGW + GD_THREADS - 1) / GD_THREADS;   // bitmap words per thread in the prefix sum (3)
constexpr int GD_LDS_TABLE_BITS = 13;                          // the largest table kept in LDS: 8192 slots of 8 bytes
constexpr unsigned long long GD_EMPTY = ~0ull;
constexpr uint32_t GD_LIVE = 0xffffffffu;                      // s_dv: the entry is not in D

__device__ __forceinline__ bool bit_of(const uint32_t* words, uint32_t id) { return (words[id >> 5] >> (id & 31)) & 1u; }

// slots of the walk's table: a power of two, at least 1.5 x the entries the walk can contribute
inline int walk_table_bits(size_t walk) {
    int bits = 6;
    while (((size_t)1 << bits) < walk + walk / 2 + 1) bits++;
    return bits;
}

// One workgroup per 32-node word of the bitmaps, one wave per list (eight lists per wave, one after another).
__global__ __launch_bounds__(GD_THREADS) void delete_mark_kernel(const uint32_t* __restrict__ adj, const uint32_t* __restrict__ deg, uint32_t n, int S,
                                                                 const uint32_t* __restrict__ dbits, const uint32_t* __restrict__ deleted,
                                                                 uint32_t* __restrict__ affected, uint32_t* err, uint32_t* n_new) {
    __shared__ uint32_t s_part[GD_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x;
    uint32_t bits = 0;
    bool bad = false;
    for (int i = 0; i < 8; i++) {
        const uint32_t p = w * 32u + (uint32_t)(wave * 8 + i);   // the same in every lane
        if (p >= n) break;
        uint32_t dg = deg[p];   // (the lists of D's own members are read too: the gather walks them, so they are validated here)
        if (dg > (uint32_t)S) { bad = true; dg = (uint32_t)S; }
        bool hit = false;
        for (uint32_t e = (uint32_t)lane; e < dg; e += 64) {
            const uint32_t v = adj[(size_t)p * S + e];
            if (v >= n) bad = true;
            else hit |= bit_of(dbits, v);
        }
        if (__ballot(hit) && !bit_of(dbits, p)) bits |= 1u << (wave * 8 + i);
    }
    if (lane == 0) s_part[wave] = bits;
    if (__ballot(bad) && lane == 0) atomicOr(err, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        affected[w] = s_part[0] | s_part[1] | s_part[2] | s_part[3];
        const uint32_t fresh = dbits[w] & ~(deleted ? deleted[w] : 0u);   // (a filter has no bit past its last row)
        if (fresh) atomicAdd(n_new, (uint32_t)__popc(fresh));
    }
}

__global__ void delete_check_ids_kernel(const uint32_t* __restrict__ ids, size_t n_ids, const uint32_t* __restrict__ dbits, uint32_t* hit) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ids && bit_of(dbits, ids[i])) atomicOr(hit, 1u);
}

struct GatherArgs {
    const uint16_t* base; uint32_t n; int d;
    const uint32_t* adj; const uint32_t* deg; int S;
    const uint32_t* dbits;
    const uint32_t* points;
    uint32_t* cand_ids; long long* cand_sc; uint32_t cap;
    uint32_t* counts;
    unsigned long long* table; int table_bits;   // table: one (1 << table_bits)-slot table per workgroup in HBM, or null (LDS)
    int maxc;
    uint32_t* stats;   // [0] longest candidate list, [1] lists longer than maxc
    uint32_t* err;     // bit 0: an edge outside the graph; bit 1: the table overflowed (cannot happen: it is sized for the whole walk)
};

inline size_t gather_fixed_lds(int d) { return (size_t)((d * 2 + 15) & ~15) + GD_SMAX * 8 + GD_FLAGW * 8 + GD_THREADS * 4; }

// A slot holds (id << 32 | walk position); all values that ever meet in one slot carry the same id, so the 64-bit minimum is the
// smallest position.  Read with an atomic load: in HBM the table is written by atomics, which a cached plain load need not see.
__device__ __forceinline__ unsigned long long slot_load(const unsigned long long* p) {
    return __hip_atomic_load(const_cast<unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS_TABLE>
__global__ __launch_bounds__(GD_THREADS) void delete_gather_kernel(GatherArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dq = (a.d * 2 + 15) & ~15;
    uint16_t* s_q = reinterpret_cast<uint16_t*>(smem);
    char* p0 = smem + dq;
    uint32_t* s_np = reinterpret_cast<uint32_t*>(p0); p0 += GD_SMAX * 4;     // N(p)
    uint32_t* s_dv = reinterpret_cast<uint32_t*>(p0); p0 += GD_SMAX * 4;     // per entry: GD_LIVE, or the length of the deleted entry's list
    uint32_t* s_flag = reinterpret_cast<uint32_t*>(p0); p0 += GD_FLAGW * 4;  // walk positions that survive
    uint32_t* s_pre = reinterpret_cast<uint32_t*>(p0); p0 += GD_FLAGW * 4;   // survivors before each bitmap word
    uint32_t* s_scan = reinterpret_cast<uint32_t*>(p0); p0 += GD_THREADS * 4;
    unsigned long long* table;
    if constexpr (LDS_TABLE) table = reinterpret_cast<unsigned long long*>(p0);
    else table = a.table + (size_t)blockIdx.x * ((size_t)1 << a.table_bits);
    __shared__ int s_walk, s_nc;

    const int tid = threadIdx.x, S = a.S, d = a.d;
    const size_t bi = blockIdx.x;
    const uint32_t p = a.points[bi];
    uint32_t* ci = a.cand_ids + bi * (size_t)a.cap;
    long long* cs = a.cand_sc + bi * (size_t)a.cap;
    int dp = (int)a.deg[p];
    if (dp > S) dp = S;

    for (int e = tid; e < d / 8; e += GD_THREADS) reinterpret_cast<uint4*>(s_q)[e] = reinterpret_cast<const uint4*>(a.base + (size_t)p * d)[e];
    if (tid == 0) s_walk = 0;
    __syncthreads();
    if (tid < dp) {
        uint32_t v = a.adj[(size_t)p * S + tid], dv = GD_LIVE;
        int contributes = 1;
        if (v >= a.n) {   // reported; stands for p itself, which the walk drops
            atomicOr(a.err, 1u);
            v = p;
        } else if (bit_of(a.dbits, v)) {
            dv = a.deg[v];
            if (dv > (uint32_t)S) dv = (uint32_t)S;
            contributes = (int)dv;
        }
        s_np[tid] = v;
        s_dv[tid] = dv;
        atomicAdd(&s_walk, contributes);
    }
    __syncthreads();
    // the table is sized for this node's walk (most nodes list one or two deleted rows), within what the launch provides
    const int walk = s_walk;
    int tb = 6;
    while ((1 << tb) < walk + (walk >> 1) + 1 && tb < a.table_bits) tb++;
    const uint32_t slots = 1u << tb, mask = slots - 1u;
    const int npos = dp * (S + 1), nfw = (npos + 31) >> 5;   // walk position of entry j: j (S + 1); of entry k of a deleted entry j: j (S + 1) + 1 + k
    for (uint32_t h = (uint32_t)tid; h < slots; h += GD_THREADS) table[h] = GD_EMPTY;
    for (int e = tid; e < nfw; e += GD_THREADS) s_flag[e] = 0u;
    __syncthreads();

    for (int pos = tid; pos < npos; pos += GD_THREADS) {
        const int j = pos / (S + 1), k = pos - j * (S + 1);
        const uint32_t v = s_np[j], dv = s_dv[j];
        uint32_t c;
        if (k == 0) {
            if (dv != GD_LIVE) continue;
            c = v;
        } else {
            if (dv == GD_LIVE || (uint32_t)(k - 1) >= dv) continue;
            c = a.adj[(size_t)v * S + (k - 1)];
            if (c >= a.n) { atomicOr(a.err, 1u); continue; }
            if (bit_of(a.dbits, c)) continue;
        }
        if (c == p) continue;
        const unsigned long long key = ((unsigned long long)c << 32) | (uint32_t)pos;
        uint32_t h = (c * 2654435761u) >> (32 - tb);
        uint32_t probe = 0;
        for (; probe < slots; probe++) {
            const unsigned long long prev = atomicCAS(&table[h], GD_EMPTY, key);
            if (prev == GD_EMPTY) break;
            if ((uint32_t)(prev >> 32) == c) {
                if (key < prev) atomicMin(&table[h], key);
                break;
            }
            h = (h + 1u) & mask;
        }
        if (probe == slots) atomicOr(a.err, 2u);
    }
    __syncthreads();
    for (uint32_t h = (uint32_t)tid; h < slots; h += GD_THREADS) {
        const unsigned long long v = slot_load(&table[h]);
        if (v != GD_EMPTY) atomicOr(&s_flag[(uint32_t)v >> 5], 1u << ((uint32_t)v & 31u));
    }
    __syncthreads();
    {   // survivors before each bitmap word: a thread owns GD_WPT consecutive words
        uint32_t mine = 0;
        for (int x = 0; x < GD_WPT; x++) {
            const int w = tid * GD_WPT + x;
            if (w < nfw) mine += (uint32_t)__popc(s_flag[w]);
        }
        s_scan[tid] = mine;
        __syncthreads();
        for (int off = 1; off < GD_THREADS; off <<= 1) {
            const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        uint32_t run = s_scan[tid] - mine;
        for (int x = 0; x < GD_WPT; x++) {
            const int w = tid * GD_WPT + x;
            if (w < nfw) { s_pre[w] = run; run += (uint32_t)__popc(s_flag[w]); }
        }
        if (tid == GD_THREADS - 1) s_nc = (int)s_scan[tid];
    }
    __syncthreads();
    int nc = s_nc;
    if (nc > (int)a.cap) nc = (int)a.cap;   // (cap covers the longest possible walk)
    for (uint32_t h = (uint32_t)tid; h < slots; h += GD_THREADS) {
        const unsigned long long v = slot_load(&table[h]);
        if (v == GD_EMPTY) continue;
        const uint32_t pos = (uint32_t)v;
        const uint32_t rank = s_pre[pos >> 5] + (uint32_t)__popc(s_flag[pos >> 5] & ((1u << (pos & 31u)) - 1u));
        if (rank < (uint32_t)nc) ci[rank] = (uint32_t)(v >> 32);
    }
    __syncthreads();
    for (int e0 = 0; e0 < nc; e0 += GD_THREADS / 4) {   // fast_dot(row p, row c), one lane quad per candidate
        const int e = e0 + (tid >> 2);
        const uint32_t id = ci[e < nc ? e : nc - 1];
        const float f = quad_fast_dot_f32(a.base + (size_t)id * d, s_q, d);
        if (e < nc && (tid & 3) == 0) cs[e] = scale_dot_result(f);
    }
    if (tid == 0) {
        a.counts[bi] = (uint32_t)nc;
        atomicMax(&a.stats[0], (uint32_t)nc);
        if (nc > a.maxc) atomicAdd(&a.stats[1], 1u);
    }
}

__global__ void delete_finish_kernel(uint32_t* __restrict__ deg, uint8_t* __restrict__ has_url, uint32_t* __restrict__ deleted,
                                     const uint32_t* __restrict__ dbits, size_t n_words) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint32_t b = dbits[w];
    if (!b) return;
    deleted[w] |= b;
    while (b) {
        const size_t v = w * 32 + (size_t)(__ffs(b) - 1);
        deg[v] = 0u;
        has_url[v] = 0;
        b &= b - 1u;
    }
}

__global__ void delete_restore_kernel(uint8_t* __restrict__ has_url, uint32_t* deleted, const uint32_t* __restrict__ ids, size_t n_ids) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ids) return;
    const uint32_t id = ids[i];
    atomicAnd(&deleted[id >> 5], ~(1u << (id & 31)));
    has_url[id] = 1;
}

}  // namespace

namespace mse {

int launch_delete_mark(const uint32_t* adj, const uint32_t* deg, size_t n, int stride, const uint32_t* dbits, const uint32_t* deleted,
                       uint32_t* affected, uint32_t* err, uint32_t* n_new, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(delete_mark_kernel, dim3((unsigned)((n + 31) / 32)), dim3(GD_THREADS), 0, stream, adj, deg, (uint32_t)n, stride, dbits, deleted,
                       affected, err, n_new);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_delete_check_ids(const uint32_t* ids, size_t n_ids, const uint32_t* dbits, uint32_t* hit, hipStream_t stream) {
    if (n_ids == 0) return 0;
    hipLaunchKernelGGL(delete_check_ids_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, stream, ids, n_ids, dbits, hit);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

size_t delete_gather_table_bytes(int stride, size_t nb) {
    const int bits = walk_table_bits((size_t)stride + (size_t)stride * stride);
    return bits <= GD_LDS_TABLE_BITS ? 0 : nb * ((size_t)8 << bits);
}

int launch_delete_gather(const uint16_t* base, size_t n, int d, const uint32_t* adj, const uint32_t* deg, int stride, const uint32_t* dbits,
                         const uint32_t* points, size_t nb, uint32_t* cand_ids, long long* cand_sc, size_t cap, uint32_t* counts, void* table,
                         int maxc, uint32_t* stats, uint32_t* err, hipStream_t stream) {
    if (nb == 0) return 0;
    if (stride < 1 || stride > GD_SMAX || cap < (size_t)stride + (size_t)stride * stride || cap > 0xffffffffull) return fail("delete_gather: bad stride / capacity");
    GatherArgs a{};
    a.base = base; a.n = (uint32_t)n; a.d = d;
    a.adj = adj; a.deg = deg; a.S = stride;
    a.dbits = dbits; a.points = points;
    a.cand_ids = cand_ids; a.cand_sc = cand_sc; a.cap = (uint32_t)cap; a.counts = counts;
    a.table_bits = walk_table_bits((size_t)stride + (size_t)stride * stride);
    a.maxc = maxc; a.stats = stats; a.err = err;
    if (a.table_bits <= GD_LDS_TABLE_BITS) {
        const size_t lds = gather_fixed_lds(d) + ((size_t)8 << a.table_bits);
        MSE_DYN_LDS(delete_gather_kernel<true>, 96 * 1024);
        hipLaunchKernelGGL(delete_gather_kernel<true>, dim3((unsigned)nb), dim3(GD_THREADS), lds, stream, a);
    } else {
        if (!table) return fail("delete_gather: no table scratch");
        a.table = reinterpret_cast<unsigned long long*>(table);
        MSE_DYN_LDS(delete_gather_kernel<false>, 96 * 1024);
        hipLaunchKernelGGL(delete_gather_kernel<false>, dim3((unsigned)nb), dim3(GD_THREADS), gather_fixed_lds(d), stream, a);
    }
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_delete_finish(uint32_t* deg, uint8_t* has_url, uint32_t* deleted, const uint32_t* dbits, size_t n, hipStream_t stream) {
    const size_t n_words = (n + 31) / 32;
    if (n_words == 0) return 0;
    hipLaunchKernelGGL(delete_finish_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, deg, has_url, deleted, dbits, n_words);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_delete_restore(uint8_t* has_url, uint32_t* deleted, const uint32_t* ids, size_t n_ids, hipStream_t stream) {
    if (n_ids == 0) return 0;
    hipLaunchKernelGGL(delete_restore_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, stream, has_url, deleted, ids, n_ids);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mse

namespace {

// the per-graph arrays a delete needs, made on first use: has_url (all ones) and the deleted map (all zeros)
int ensure_delete_state(mse_graph* g, hipStream_t st) {
    const size_t n_words = (g->n + 31) / 32;
    if (!g->has_url) {
        uint8_t* hu = nullptr;
        MSE_HIP_TRY(hipMalloc((void**)&hu, g->n));
        hipError_t e = hipMemsetAsync(hu, 1, g->n, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(hu); return fail(std::string("graph_delete_rows: ") + hipGetErrorString(e)); }
        g->has_url = hu;
    }
    if (!g->deleted) {
        uint32_t* dl = nullptr;
        MSE_HIP_TRY(hipMalloc((void**)&dl, n_words * 4));
        hipError_t e = hipMemsetAsync(dl, 0, n_words * 4, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(dl); return fail(std::string("graph_delete_rows: ") + hipGetErrorString(e)); }
        g->deleted = dl;
        g->n_deleted = 0;
    }
    return 0;
}

// the graph's arrays say which device they live on: the calls below make it the thread's current one, as the base's entry points do
int set_graph_device(const mse_graph* g, const char* who) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, g->adj) != hipSuccess) { (void)hipGetLastError(); return fail(std::string(who) + ": the graph's arrays are not device memory"); }
    MSE_HIP_TRY(hipSetDevice(at.device));
    return 0;
}

}  // namespace

extern "C" {

int mse_graph_delete_rows(mse_searcher* s, mse_graph* g, const mse_filter* deleted, const mse_build_config* cfg, size_t batch, uint64_t stats[4]) {
    if (!s || !s->base || !g || !deleted || !cfg || !stats) return fail("graph_delete_rows: null argument");
    const mse_base* b = s->base;
    if (g->n != b->n) return fail("graph_delete_rows: graph and vectors differ in length");
    if (deleted->n_rows != g->n) return fail("graph_delete_rows: the filter speaks for " + std::to_string(deleted->n_rows) + " rows, the graph has " + std::to_string(g->n));
    if (check_filter(b, deleted)) return -1;
    if (b->n >= 0xffffffffull) return fail("graph_delete_rows: too many vectors");
    if (g->max_deg > (size_t)GD_SMAX) return fail("graph_delete_rows: at most 128 neighbours per node");
    if (cfg->r == 0 || cfg->r > 64 || cfg->r > g->max_deg) return fail("graph_delete_rows: r must be 1..64 and at most the graph's stride");
    if (cfg->maxc == 0 || cfg->maxc > 1024) return fail("graph_delete_rows: maxc must be 1..1024");
    if (b->d == 0 || b->d % 32 || b->d > 4096) return fail("graph_delete_rows: vector width must be a multiple of 32");
    // exclusive: waits for the request-path calls in flight on the graph (they hold the lock shared) and keeps new ones out
    std::lock_guard<SharedExclusive> ex(g->entry_lock);
    MSE_HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    const size_t n = g->n, n_words = (n + 31) / 32;
    const int S = (int)g->max_deg, r = (int)cfg->r, d = (int)b->d;
    for (int i = 0; i < 4; i++) stats[i] = 0;
    if (deleted->count == 0) return 0;

    // words: [0] bad edge, [1] rows newly deleted, [2] an entry node in D, [3] longest candidate list, [4] lists over maxc, [5] prune, [6] gather
    // scratch lives on the searcher and is kept between calls: a hipFree is a device-wide wait, and this call holds the graph's lock
    DevBuf &wrd = s->del_scratch[0], &aff = s->del_scratch[1], &aff_ids = s->del_scratch[2], &cscr = s->del_scratch[3];
    if (wrd.ensure(64) || aff.ensure(n_words * 4) || cscr.ensure(filter_compact_scratch_bytes(n_words) + 16)) return -1;
    uint32_t* w = wrd.as<uint32_t>();
    MSE_HIP_TRY(hipMemsetAsync(w, 0, 64, st));
    if (g->n_entries && g->entry_ids && launch_delete_check_ids(g->entry_ids, g->n_entries, deleted->words, w + 2, st)) return -1;
    if (launch_delete_mark(g->adj, g->deg, n, S, deleted->words, g->deleted, aff.as<uint32_t>(), w, w + 1, st)) return -1;
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    MSE_HIP_TRY(hipMemcpyAsync(h, w, 32, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (h[2]) return fail("graph_delete_rows: a node of the graph's entry table is in the delete set (move the entry first: mse_graph_set_entries)");
    if (h[0]) return fail("graph_delete_rows: the graph has an edge outside 0..n or a list longer than its stride");
    const size_t n_new = h[1];
    // the affected nodes, ascending
    size_t n_aff_max = n - std::min(n, deleted->count);
    if (aff_ids.ensure(std::max<size_t>(n_aff_max, 1) * 4)) return -1;
    unsigned long long* cnt_dev = reinterpret_cast<unsigned long long*>(cscr.as<char>() + ((filter_compact_scratch_bytes(n_words) + 7) & ~(size_t)7));
    if (launch_filter_compact(aff.as<uint32_t>(), n_words, aff_ids.as<uint32_t>(), cnt_dev, cscr.p, st)) return -1;
    unsigned long long n_aff = 0;
    MSE_HIP_TRY(hipMemcpyAsync(&n_aff, cnt_dev, 8, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (ensure_delete_state(g, st)) return -1;   // (nothing a search can tell from before: all urls, nothing deleted)

    if (n_aff) {
        const size_t cap = (size_t)S + (size_t)S * S;
        const size_t per_node = cap * 12 + delete_gather_table_bytes(S, 1) + (size_t)r * 4 + 8;
        if (batch == 0) batch = std::min<size_t>(8192, std::max<size_t>(64, ((size_t)1 << 28) / per_node));
        batch = std::min<size_t>(std::min<size_t>(batch, 65536), (size_t)n_aff);
        DevBuf &cid = s->del_scratch[4], &csc = s->del_scratch[5], &cnt = s->del_scratch[6], &tab = s->del_scratch[7], &stg = s->del_scratch[8],
               &stg_len = s->del_scratch[9];
        if (cid.ensure(batch * cap * 4) || csc.ensure(batch * cap * 8) || cnt.ensure(batch * 4) || stg.ensure(batch * r * 4) || stg_len.ensure(batch * 4)) return -1;
        const size_t tab_bytes = delete_gather_table_bytes(S, batch);
        if (tab_bytes && tab.ensure(tab_bytes)) return -1;
        PruneLaunch pl{b->dev, (uint32_t)n, d, cfg->query_breakpoint, cfg->alpha, cfg->query_alpha, r, (int)cfg->maxc, (int)cfg->saturate_graph, 0, w + 5};
        if (prune_mfma_eps(b, cfg, st, &pl.eps_fix)) return -1;
        for (size_t b0 = 0; b0 < n_aff; b0 += batch) {
            const size_t nb = std::min<size_t>(batch, n_aff - b0);
            const uint32_t* pts = aff_ids.as<uint32_t>() + b0;
            if (launch_delete_gather(b->dev, n, d, g->adj, g->deg, S, deleted->words, pts, nb, cid.as<uint32_t>(), csc.as<long long>(), cap, cnt.as<uint32_t>(),
                                     tab.p, (int)cfg->maxc, w + 3, w + 6, st) ||
                launch_prune_lists(pl, cid.as<uint32_t>(), csc.as<long long>(), cap, cnt.as<uint32_t>(), pts, stg.as<uint32_t>(), stg_len.as<uint32_t>(), nb, st) ||
                launch_apply_lists(g->adj, g->deg, (size_t)S, r, pts, stg.as<uint32_t>(), stg_len.as<uint32_t>(), nb, st))
                return -1;
        }
    }
    if (launch_delete_finish(g->deg, g->has_url, g->deleted, deleted->words, n, st)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(h, w, 32, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    g->n_deleted += n_new;
    stats[0] = n_new; stats[1] = n_aff; stats[2] = h[3]; stats[3] = h[4];
    if (h[5] || h[6]) return fail("graph_delete_rows: internal error " + std::to_string(h[5]) + "/" + std::to_string(h[6]) + " (a candidate id outside the index)");
    return 0;
}

int mse_graph_deleted(const mse_graph* g, uint8_t* out_or_null, size_t* count) {
    if (!g) return fail("graph_deleted: null argument");
    // (shared: a delete in flight on another thread is either wholly before or wholly after this answer)
    g->entry_lock.lock_shared();
    struct Hold { SharedExclusive& l; ~Hold() { l.unlock_shared(); } } hold{g->entry_lock};
    if (count) *count = g->n_deleted;
    if (!out_or_null) return 0;
    if (!g->deleted) { memset(out_or_null, 0, g->n); return 0; }
    if (set_graph_device(g, "graph_deleted")) return -1;
    std::vector<uint32_t> words((g->n + 31) / 32);
    MSE_HIP_TRY(hipMemcpyAsync(words.data(), g->deleted, words.size() * 4, hipMemcpyDeviceToHost, hipStreamPerThread));
    MSE_HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    for (size_t i = 0; i < g->n; i++) out_or_null[i] = (uint8_t)((words[i >> 5] >> (i & 31)) & 1u);
    return 0;
}

int mse_graph_restore_rows(mse_graph* g, const uint32_t* ids, size_t n_ids) {
    if (!g || (n_ids && !ids)) return fail("graph_restore_rows: null argument");
    if (n_ids == 0) return 0;
    std::lock_guard<SharedExclusive> ex(g->entry_lock);
    if (set_graph_device(g, "graph_restore_rows")) return -1;
    hipStream_t st = hipStreamPerThread;   // (the exclusive lock has drained the request path; the graph's arrays are idle)
    std::vector<uint32_t> words((g->n + 31) / 32, 0u);
    if (g->deleted) {
        MSE_HIP_TRY(hipMemcpyAsync(words.data(), g->deleted, words.size() * 4, hipMemcpyDeviceToHost, st));
        MSE_HIP_TRY(hipStreamSynchronize(st));
    }
    for (size_t i = 0; i < n_ids; i++) {   // every id once, and deleted: found before anything changes
        const uint32_t id = ids[i];
        if (id >= g->n) return fail("graph_restore_rows: id " + std::to_string(id) + " is outside the graph");
        if (!((words[id >> 5] >> (id & 31)) & 1u)) return fail("graph_restore_rows: row " + std::to_string(id) + " is not deleted (or is named twice)");
        words[id >> 5] &= ~(1u << (id & 31));
    }
    DevBuf d_ids;
    if (d_ids.ensure(n_ids * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(d_ids.p, ids, n_ids * 4, hipMemcpyHostToDevice, st));
    if (launch_delete_restore(g->has_url, g->deleted, d_ids.as<uint32_t>(), n_ids, st)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(st));   // (before d_ids is freed and the lock released)
    g->n_deleted -= n_ids;
    return 0;
}

}  // extern "C"
