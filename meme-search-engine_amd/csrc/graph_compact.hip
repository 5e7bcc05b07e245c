// Repack a live graph index into a fresh (base, codes, graph) triple of a chosen capacity (include/mse.h "compact deleted rows away and
// grow capacity"): live rows renumbered densely in their old order, the spare tail marked deleted for mse_graph_insert_rows.  Out of
// place: the old handles are only read.  Three steps under the old graph's entry lock, held SHARED:
//   map     compact_live_kernel       the live bitmap (NOT deleted, rows past n cleared); the filter compaction (filter.hip) turns it into
//                                     the ascending list of live ids = new_to_old; compact_scatter_kernel inverts it into old_to_new.  Both
//                                     maps are 0xFF-filled first, so deleted rows and spare slots read 0xFFFFFFFF.
//   gather  compact_gather_kernel     one wave per destination row, four rows per wave, the pieces of all four loaded before the first is
//                                     stored (twelve 16-byte loads per lane in flight at d = 1152): row-contiguous reads at scattered row
//                                     addresses, fully contiguous writes.  The row's code and descriptor bytes ride along; rows of the
//                                     spare tail are written as zeros.
//   remap   compact_remap_kernel      one workgroup per 32 new nodes, one wave per list (eight lists per wave, as delete_mark_kernel walks
//                                     them): every entry below deg through old_to_new to the same position of the new list, zeros behind
//                                     it (what mse_graph_new leaves in an entry never written); deg, has_url, the word of the new deleted
//                                     map; an entry outside the graph or mapped to 0xFFFFFFFF raises the one error word, read before
//                                     anything is handed back.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <cstring>
#include <new>

using namespace mse;

namespace {

constexpr int CG_ROWS = 4;     // destination rows per wave, all in flight together
constexpr int CG_PIECES = 3;   // 16-byte pieces per lane and row in one sweep: 192 pieces = 3072 bytes (d = 1152: 144 pieces, one sweep)

__global__ void compact_live_kernel(const uint32_t* __restrict__ deleted /* or null */, size_t n, size_t n_words, uint32_t* __restrict__ live) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint32_t v = deleted ? ~deleted[w] : 0xffffffffu;
    const size_t r0 = w * 32;
    if (r0 + 32 > n) v &= r0 < n ? (0xffffffffu >> (32 - (n - r0))) : 0u;
    live[w] = v;
}

__global__ void compact_scatter_kernel(const uint32_t* __restrict__ new_to_old, size_t n_live, uint32_t n, uint32_t* __restrict__ old_to_new) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    const uint32_t old = new_to_old[i];
    if (old < n) old_to_new[old] = (uint32_t)i;   // (the compaction names set bits of the live map only: always below n)
}

struct GatherArgs {
    const uint16_t* src; uint16_t* dst; int pieces;    // pieces: 16-byte pieces per row (d / 8)
    const uint8_t* codes_src; uint8_t* codes_dst; int cs;   // or null
    const uint8_t* desc_src; uint8_t* desc_dst; int nd;     // or null
    const uint32_t* new_to_old; uint32_t n, n_live, capacity;
};

// the (at most) CG_PIECES pieces of one row that belong to this lane in the sweep that starts at piece e0: loaded (zeros for a spare slot), stored
struct RowPieces { uint4 v[CG_PIECES]; };
__device__ __forceinline__ RowPieces load_pieces(const uint4* __restrict__ src, uint32_t old, int pieces, int e0, int lane) {
    RowPieces r;
    const uint4* sp = src + (size_t)(old == ID_NONE ? 0u : old) * pieces;
#pragma unroll
    for (int p = 0; p < CG_PIECES; p++) {
        const int e = e0 + p * 64 + lane;
        r.v[p] = make_uint4(0u, 0u, 0u, 0u);
        if (old != ID_NONE && e < pieces) r.v[p] = sp[e];
    }
    return r;
}
__device__ __forceinline__ void store_pieces(uint4* __restrict__ dst, size_t nw, bool in, const RowPieces& r, int pieces, int e0, int lane) {
    uint4* dp = dst + nw * pieces;
#pragma unroll
    for (int p = 0; p < CG_PIECES; p++) {
        const int e = e0 + p * 64 + lane;
        if (in && e < pieces) dp[e] = r.v[p];
    }
}
// the source of destination row nw (the same in every lane); a spare slot, or a row past the capacity, has none
__device__ __forceinline__ uint32_t source_row(const uint32_t* __restrict__ new_to_old, size_t nw, uint32_t n_live, uint32_t n) {
    const uint32_t o = nw < n_live ? new_to_old[nw] : ID_NONE;
    return o < n ? o : ID_NONE;
}

// code and descriptor bytes of destination row nw from source row o (ID_NONE: zeros)
__device__ __forceinline__ void move_small(const GatherArgs& a, size_t nw, bool in, uint32_t o, int lane) {
    if (!in) return;
    if (a.codes_dst) {
        const int cs = a.cs;
        uint8_t* cd = a.codes_dst + nw * cs;
        const uint8_t* csrc = a.codes_src + (size_t)(o == ID_NONE ? 0u : o) * cs;
        if ((cs & 15) == 0) {   // (both slabs are 16-byte aligned: hipMalloc, and rows of a multiple of 16 bytes)
            for (int e = lane; e < cs / 16; e += 64) {
                uint4 c = make_uint4(0u, 0u, 0u, 0u);
                if (o != ID_NONE) c = reinterpret_cast<const uint4*>(csrc)[e];
                reinterpret_cast<uint4*>(cd)[e] = c;
            }
        } else {
            for (int e = lane; e < cs; e += 64) {
                uint8_t c = 0;
                if (o != ID_NONE) c = csrc[e];
                cd[e] = c;
            }
        }
    }
    if (a.desc_dst) {
        const int nd = a.nd;
        for (int e = lane; e < nd; e += 64) {
            uint8_t c = 0;
            if (o != ID_NONE) c = a.desc_src[(size_t)o * nd + e];
            a.desc_dst[nw * nd + e] = c;
        }
    }
}

__global__ __launch_bounds__(256) void compact_gather_kernel(GatherArgs a) {
    static_assert(CG_ROWS == 4, "the four rows of a wave are written out by name");
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t row0 = wave * CG_ROWS;
    if (row0 >= a.capacity) return;
    const uint32_t o0 = source_row(a.new_to_old, row0, a.n_live, a.n), o1 = source_row(a.new_to_old, row0 + 1, a.n_live, a.n),
                   o2 = source_row(a.new_to_old, row0 + 2, a.n_live, a.n), o3 = source_row(a.new_to_old, row0 + 3, a.n_live, a.n);
    const bool in1 = row0 + 1 < a.capacity, in2 = row0 + 2 < a.capacity, in3 = row0 + 3 < a.capacity;
    const uint4* src = reinterpret_cast<const uint4*>(a.src);
    uint4* dst = reinterpret_cast<uint4*>(a.dst);
    for (int e0 = 0; e0 < a.pieces; e0 += 64 * CG_PIECES) {
        const RowPieces r0 = load_pieces(src, o0, a.pieces, e0, lane), r1 = load_pieces(src, o1, a.pieces, e0, lane),
                        r2 = load_pieces(src, o2, a.pieces, e0, lane), r3 = load_pieces(src, o3, a.pieces, e0, lane);
        store_pieces(dst, row0, true, r0, a.pieces, e0, lane);
        store_pieces(dst, row0 + 1, in1, r1, a.pieces, e0, lane);
        store_pieces(dst, row0 + 2, in2, r2, a.pieces, e0, lane);
        store_pieces(dst, row0 + 3, in3, r3, a.pieces, e0, lane);
    }
    if (!a.codes_dst && !a.desc_dst) return;
    move_small(a, row0, true, o0, lane);   // (64 + 4 bytes a row beside the 2304 above: one row after another)
    move_small(a, row0 + 1, in1, o1, lane);
    move_small(a, row0 + 2, in2, o2, lane);
    move_small(a, row0 + 3, in3, o3, lane);
}

struct RemapArgs {
    const uint32_t* adj; const uint32_t* deg; const uint8_t* has_url /* or null */; int S;
    uint32_t* adj_new; uint32_t* deg_new; uint8_t* has_url_new /* or null */; uint32_t* deleted_new /* or null */;
    const uint32_t* new_to_old; const uint32_t* old_to_new;
    uint32_t n, n_live, capacity;
    uint32_t* err; unsigned long long* edges;
};

// One workgroup per 32-node word of the new deleted map, one wave per list (eight lists per wave, one after another).
__global__ __launch_bounds__(256) void compact_remap_kernel(RemapArgs a) {
    __shared__ unsigned long long s_edges[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w = blockIdx.x;
    const int S = a.S;
    unsigned long long edges = 0;
    bool bad = false;
    for (int i = 0; i < 8; i++) {
        const size_t nw = (size_t)w * 32 + (size_t)(wave * 8 + i);   // the same in every lane
        if (nw >= a.capacity) break;
        uint32_t old = nw < a.n_live ? a.new_to_old[nw] : ID_NONE;
        if (old != ID_NONE && old >= a.n) { bad = true; old = ID_NONE; }
        uint32_t dg = 0;
        if (old != ID_NONE) {
            dg = a.deg[old];
            if (dg > (uint32_t)S) { bad = true; dg = (uint32_t)S; }
        }
        for (int e = lane; e < S; e += 64) {
            uint32_t m = 0u;
            if ((uint32_t)e < dg) {
                const uint32_t v = a.adj[(size_t)old * S + e];
                if (v >= a.n) bad = true;
                else {
                    m = a.old_to_new[v];
                    if (m == ID_NONE) { bad = true; m = 0u; }
                }
            }
            a.adj_new[nw * S + e] = m;
        }
        if (lane == 0) {
            a.deg_new[nw] = dg;
            if (a.has_url_new) a.has_url_new[nw] = old == ID_NONE ? (uint8_t)0 : (a.has_url ? a.has_url[old] : (uint8_t)1);
        }
        edges += dg;
    }
    if (lane == 0) s_edges[wave] = edges;
    if (__ballot(bad) && lane == 0) atomicOr(a.err, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long e = s_edges[0] + s_edges[1] + s_edges[2] + s_edges[3];
        if (e) atomicAdd(a.edges, e);
        if (a.deleted_new) {   // the spare tail: new ids n_live .. capacity - 1
            const size_t r0 = (size_t)w * 32;
            uint32_t bits = 0u;
            for (int b = 0; b < 32; b++)
                if (r0 + b >= a.n_live && r0 + b < a.capacity) bits |= 1u << b;
            a.deleted_new[w] = bits;
        }
    }
}

// the device memory of the new triple and the call's scratch: freed on every way out unless handed over
struct Fresh {
    void* p[16] = {};
    int used = 0;
    int alloc(void** out, size_t bytes, const char* what) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) {
            (void)hipGetLastError();
            size_t f = 0, t = 0;
            if (hipMemGetInfo(&f, &t) != hipSuccess) (void)hipGetLastError();
            return fail(std::string("graph_compact: allocation of ") + std::to_string(bytes) + " bytes for " + what + " failed (" + std::to_string(f) +
                        " bytes of device memory are free; the old and the new index are resident together)");
        }
        p[used++] = q;
        *out = q;
        return 0;
    }
    void keep() { used = 0; }
    ~Fresh() {
        for (int i = 0; i < used; i++) (void)hipFree(p[i]);
    }
};

int pointer_device(const void* p, int* dev) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    *dev = at.device;
    return 0;
}

}  // namespace

extern "C" {

int mse_graph_compact(mse_searcher* s, const mse_graph* g, const mse_codes* codes, size_t capacity, mse_base** base_out, mse_codes** codes_out,
                      mse_graph** graph_out, uint32_t* old_to_new, uint32_t* new_to_old, uint64_t stats_out[4]) {
    if (!s || !s->base || !g || !base_out || !graph_out) return fail("graph_compact: null argument");
    if (codes && !codes_out) return fail("graph_compact: null argument (codes are given, but no place for the new ones)");
    if (!codes && codes_out) return fail("graph_compact: null argument (a place for new codes, but no codes are given)");
    const mse_base* b = s->base;
    if (g->n != b->n) return fail("graph_compact: graph and vectors differ in length (" + std::to_string(g->n) + " and " + std::to_string(b->n) + " rows)");
    if (b->d == 0 || b->d % 8) return fail("graph_compact: vector width must be a multiple of 8");
    if (codes && codes->n != g->n) return fail("graph_compact: the codes speak for " + std::to_string(codes->n) + " rows, the graph has " + std::to_string(g->n));
    if (capacity == 0 || capacity > 0xFFFFFFFEull) return fail("graph_compact: capacity must be 1 .. 2^32 - 2");
    if (g->n > 0xFFFFFFFEull) return fail("graph_compact: too many vectors");
    int gdev = 0;
    if (pointer_device(g->adj, &gdev)) return fail("graph_compact: the graph's arrays are not device memory");
    if (gdev != b->device) return fail("graph_compact: the graph lives on device " + std::to_string(gdev) + ", the vectors on device " + std::to_string(b->device));
    if (codes && codes->codes && (pointer_device(codes->codes, &gdev) || gdev != b->device)) return fail("graph_compact: the codes live on another device than the vectors");

    // shared: a delete or an insert on the old graph (exclusive) runs wholly before or wholly after; the request path runs beside this call
    g->entry_lock.lock_shared();
    struct Hold { SharedExclusive& l; ~Hold() { l.unlock_shared(); } } hold{g->entry_lock};
    const size_t n = g->n, n_words = (n + 31) / 32, d = b->d, S = g->max_deg;
    const size_t n_live = n - (g->deleted ? g->n_deleted : 0);
    if (capacity < n_live) return fail("graph_compact: capacity " + std::to_string(capacity) + " is below the " + std::to_string(n_live) + " live rows");
    const size_t cs = codes ? codes->code_size : 0, nd = codes ? codes->n_desc : 0;
    const bool tail = capacity > n_live;
    const size_t cap_words = (capacity + 31) / 32;
    MSE_HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;

    // ---- allocate: the new triple first (the large ones), then the scratch; nothing has been launched when one of them fails ----------
    Fresh fresh, scratch;
    void *rows_new = nullptr, *codes_new = nullptr, *desc_new = nullptr, *adj_new = nullptr, *deg_new = nullptr, *url_new = nullptr, *del_new = nullptr;
    if (fresh.alloc(&rows_new, std::max<size_t>(capacity * d * 2, 256), "the rows")) return -1;
    if (codes && fresh.alloc(&codes_new, capacity * cs + 4096, "the codes")) return -1;   // (slack as mse_codes_from_host leaves it)
    if (nd && fresh.alloc(&desc_new, capacity * nd + 256, "the descriptors")) return -1;
    if (fresh.alloc(&adj_new, capacity * S * 4, "the lists") || fresh.alloc(&deg_new, capacity * 4, "the list lengths")) return -1;
    if ((g->has_url || tail) && fresh.alloc(&url_new, capacity, "the url flags")) return -1;
    if (tail && fresh.alloc(&del_new, cap_words * 4, "the deleted map")) return -1;
    void *live = nullptr, *n2o = nullptr, *o2n = nullptr, *cscr = nullptr, *wrd = nullptr;
    const size_t n2o_len = std::max(capacity, n);   // room for every bit the live map can hold, whatever the graph's count says
    const size_t cscr_bytes = (filter_compact_scratch_bytes(n_words) + 7) & ~(size_t)7;
    if (scratch.alloc(&live, n_words * 4, "the live map") || scratch.alloc(&n2o, n2o_len * 4, "the id maps") || scratch.alloc(&o2n, n * 4, "the id maps") ||
        scratch.alloc(&cscr, cscr_bytes + 16, "the compaction") || scratch.alloc(&wrd, 32, "the counters"))
        return -1;
    unsigned long long* cnt_dev = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(cscr) + cscr_bytes);
    uint32_t* err_dev = reinterpret_cast<uint32_t*>(wrd);
    unsigned long long* edges_dev = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(wrd) + 8);

    // ---- map ---------------------------------------------------------------------------------------------------------------------------
    MSE_HIP_TRY(hipMemsetAsync(wrd, 0, 32, st));
    MSE_HIP_TRY(hipMemsetAsync(n2o, 0xff, n2o_len * 4, st));
    MSE_HIP_TRY(hipMemsetAsync(o2n, 0xff, n * 4, st));
    hipLaunchKernelGGL(compact_live_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, g->deleted, n, n_words, reinterpret_cast<uint32_t*>(live));
    MSE_HIP_TRY(hipGetLastError());
    if (launch_filter_compact(reinterpret_cast<const uint32_t*>(live), n_words, reinterpret_cast<uint32_t*>(n2o), cnt_dev, cscr, st)) return -1;
    unsigned long long counted = 0;
    MSE_HIP_TRY(hipMemcpyAsync(&counted, cnt_dev, 8, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (counted != n_live)
        return fail("graph_compact: internal error: the deleted map marks " + std::to_string(n - counted) + " rows, the graph counts " + std::to_string(n - n_live));
    if (n_live) {
        hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)((n_live + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(n2o), n_live,
                           (uint32_t)n, reinterpret_cast<uint32_t*>(o2n));
        MSE_HIP_TRY(hipGetLastError());
    }

    // ---- remap + check (before the rows: a bad list ends the call before the 2 n_live d bytes are moved) ----------------------------------
    RemapArgs ra{};
    ra.adj = g->adj; ra.deg = g->deg; ra.has_url = g->has_url; ra.S = (int)S;
    ra.adj_new = reinterpret_cast<uint32_t*>(adj_new); ra.deg_new = reinterpret_cast<uint32_t*>(deg_new);
    ra.has_url_new = reinterpret_cast<uint8_t*>(url_new); ra.deleted_new = reinterpret_cast<uint32_t*>(del_new);
    ra.new_to_old = reinterpret_cast<const uint32_t*>(n2o); ra.old_to_new = reinterpret_cast<const uint32_t*>(o2n);
    ra.n = (uint32_t)n; ra.n_live = (uint32_t)n_live; ra.capacity = (uint32_t)capacity;
    ra.err = err_dev; ra.edges = edges_dev;
    hipLaunchKernelGGL(compact_remap_kernel, dim3((unsigned)cap_words), dim3(256), 0, st, ra);
    MSE_HIP_TRY(hipGetLastError());
    uint32_t h_err = 0;
    unsigned long long h_edges = 0;
    MSE_HIP_TRY(hipMemcpyAsync(&h_err, err_dev, 4, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipMemcpyAsync(&h_edges, edges_dev, 8, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (h_err) return fail("graph_compact: a live list names a deleted row or a row outside the graph, or is longer than the graph's stride");

    // ---- gather --------------------------------------------------------------------------------------------------------------------------
    GatherArgs ga{};
    ga.src = b->dev; ga.dst = reinterpret_cast<uint16_t*>(rows_new); ga.pieces = (int)(d / 8);
    if (codes) { ga.codes_src = codes->codes; ga.codes_dst = reinterpret_cast<uint8_t*>(codes_new); ga.cs = (int)cs; }
    if (nd) { ga.desc_src = codes->desc; ga.desc_dst = reinterpret_cast<uint8_t*>(desc_new); ga.nd = (int)nd; }
    ga.new_to_old = reinterpret_cast<const uint32_t*>(n2o); ga.n = (uint32_t)n; ga.n_live = (uint32_t)n_live; ga.capacity = (uint32_t)capacity;
    const size_t rows_per_block = 4 * CG_ROWS;
    // optional measurement (mse_searcher_compact_timing): HIP events around the gather kernel alone
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (s->compact_timing) {
        MSE_HIP_TRY(hipEventCreate(&ev.e0));
        MSE_HIP_TRY(hipEventCreate(&ev.e1));
        MSE_HIP_TRY(hipEventRecord(ev.e0, st));
    }
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)((capacity + rows_per_block - 1) / rows_per_block)), dim3(256), 0, st, ga);
    MSE_HIP_TRY(hipGetLastError());
    if (ev.e1) MSE_HIP_TRY(hipEventRecord(ev.e1, st));
    if (old_to_new) MSE_HIP_TRY(hipMemcpyAsync(old_to_new, o2n, n * 4, hipMemcpyDeviceToHost, st));
    if (new_to_old) MSE_HIP_TRY(hipMemcpyAsync(new_to_old, n2o, capacity * 4, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (ev.e1) {
        float ms = 0.0f;
        MSE_HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        s->compact_gather_ms = ms;
    }

    // ---- hand over ---------------------------------------------------------------------------------------------------------------------
    mse_base* nb = new (std::nothrow) mse_base();
    mse_graph* ng = new (std::nothrow) mse_graph();
    mse_codes* nc = codes ? new (std::nothrow) mse_codes() : nullptr;
    if (!nb || !ng || (codes && !nc)) {
        delete nb; delete ng; delete nc;
        return fail("graph_compact: out of host memory");
    }
    nb->dev = reinterpret_cast<const uint16_t*>(rows_new);
    nb->n = capacity; nb->d = d; nb->owned = true; nb->n_cu = b->n_cu; nb->device = b->device;   // (the norm bound: unmeasured)
    ng->adj = reinterpret_cast<uint32_t*>(adj_new); ng->deg = reinterpret_cast<uint32_t*>(deg_new);
    ng->has_url = reinterpret_cast<uint8_t*>(url_new); ng->deleted = reinterpret_cast<uint32_t*>(del_new);
    ng->n = capacity; ng->max_deg = S; ng->n_deleted = capacity - n_live;
    if (nc) {
        nc->codes = reinterpret_cast<uint8_t*>(codes_new); nc->desc = reinterpret_cast<uint8_t*>(desc_new);
        nc->n = capacity; nc->code_size = cs; nc->n_desc = nd;
    }
    fresh.keep();
    *base_out = nb;
    *graph_out = ng;
    if (codes_out) *codes_out = nc;
    if (stats_out) {
        stats_out[0] = n_live; stats_out[1] = capacity; stats_out[2] = h_edges; stats_out[3] = (uint64_t)n_live * (d * 2 + cs + nd);
    }
    return 0;
}

int mse_searcher_compact_timing(mse_searcher* s, int enable, double* last_gather_ms) {
    if (!s) return fail("searcher_compact_timing: null argument");
    if (last_gather_ms) *last_gather_ms = s->compact_gather_ms;
    s->compact_timing = enable != 0;
    if (enable == 2 || !enable) s->compact_gather_ms = 0.0;
    return 0;
}

int mse_codes_read_rows(const mse_codes* c, size_t first, size_t n, uint8_t* codes_out, uint8_t* desc_out_or_null) {
    if (!c || (n && !codes_out)) return fail("codes_read_rows: null argument");
    if (first > c->n || n > c->n - first) return fail("codes_read_rows: row range out of bounds");
    if (desc_out_or_null && !c->n_desc) return fail("codes_read_rows: the codes carry no descriptors");
    if (n == 0) return 0;
    MSE_HIP_TRY(hipMemcpy(codes_out, c->codes + first * c->code_size, n * c->code_size, hipMemcpyDeviceToHost));
    if (desc_out_or_null) MSE_HIP_TRY(hipMemcpy(desc_out_or_null, c->desc + first * c->n_desc, n * c->n_desc, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
