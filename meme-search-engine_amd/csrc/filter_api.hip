// C ABI (include/mse.h): row filters as objects -- made from bitmaps, id lists, graphs, descriptors and scores, combined, cut and joined,
// read back.  The kernels are in filter.hip; the searches that take a filter are in bruteforce.hip, api_pq.hip and beam_search.hip.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>

namespace mse {

int check_filter(const mse_base* b, const mse_filter* f) {
    if (!f) return fail("null filter");
    if (f->n_rows > b->n) return fail("filter is longer than the base (" + std::to_string(f->n_rows) + " > " + std::to_string(b->n) + " rows)");
    if (f->device != b->device) return fail("filter was made on another device than the base's");   // no silent copy
    return 0;
}

}  // namespace mse

using namespace mse;

extern "C" {

static mse_filter* filter_alloc(size_t n_rows) {
    if (n_rows > 0xFFFFFFFEull) { fail("row ids are u32: too many rows"); return nullptr; }
    mse_filter* f = new (std::nothrow) mse_filter();
    if (!f) { fail("out of host memory"); return nullptr; }
    f->n_rows = n_rows;
    f->n_words = (n_rows + 255) / 256 * 8;   // whole 256-row scan tiles: one word per 32-row group
    if (hipGetDevice(&f->device) != hipSuccess) f->device = 0;
    if (hipMalloc((void**)&f->words, std::max<size_t>(f->n_words, 1) * 4) != hipSuccess) {
        delete f; fail("hipMalloc failed for the filter"); return nullptr;
    }
    return f;
}

// the filter's id list and count, from its bitmap (on the device); frees f on failure
static mse_filter* filter_finish(mse_filter* f) {
    DevBuf scratch;
    unsigned long long count = 0;
    hipError_t e = hipSuccess;
    if (scratch.ensure(filter_compact_scratch_bytes(f->n_words) + 8)) goto bad;
    if (hipMalloc((void**)&f->ids, std::max<size_t>(f->n_rows, 1) * 4) != hipSuccess) { fail("hipMalloc failed for the filter"); goto bad; }
    {
        unsigned long long* count_dev = scratch.as<unsigned long long>();
        if (launch_filter_compact(f->words, f->n_words, f->ids, count_dev, scratch.as<char>() + 8, nullptr)) goto bad;
        e = hipMemcpy(&count, count_dev, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { fail(std::string("filter: ") + hipGetErrorString(e)); goto bad; }
    }
    f->count = (size_t)count;
    return f;
bad:
    mse_filter_free(f);
    return nullptr;
}

mse_filter* mse_filter_from_bits(const uint8_t* bits, size_t n_rows) {
    if (!bits && n_rows) { fail("null bitmap"); return nullptr; }
    mse_filter* f = filter_alloc(n_rows);
    if (!f) return nullptr;
    std::vector<uint32_t> w(std::max<size_t>(f->n_words, 1), 0u);
    if (n_rows) {
        std::memcpy(w.data(), bits, (n_rows + 7) / 8);   // LSB-first bytes = little-endian words
        if (n_rows % 32) w[n_rows / 32] &= (1u << (n_rows % 32)) - 1u;   // no bit past the last row
    }
    if (hipMemcpy(f->words, w.data(), w.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        mse_filter_free(f); fail("hipMemcpy failed for the filter"); return nullptr;
    }
    return filter_finish(f);
}

mse_filter* mse_filter_from_ids(const uint32_t* ids, size_t n_ids, size_t n_rows) {
    if (!ids && n_ids) { fail("null id array"); return nullptr; }
    for (size_t i = 0; i < n_ids; i++)
        if (ids[i] >= n_rows) { fail("filter: id " + std::to_string(ids[i]) + " is not below n_rows " + std::to_string(n_rows)); return nullptr; }
    mse_filter* f = filter_alloc(n_rows);
    if (!f) return nullptr;
    // all on the null stream: the blocking read-back of the count in filter_finish orders the OR kernel and the compaction
    DevBuf idb;
    if (idb.ensure(std::max<size_t>(n_ids, 1) * 4)) { mse_filter_free(f); return nullptr; }
    if (hipMemset(f->words, 0, std::max<size_t>(f->n_words, 1) * 4) != hipSuccess ||
        (n_ids && hipMemcpy(idb.p, ids, n_ids * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        mse_filter_free(f);
        fail("filter: device upload failed");
        return nullptr;
    }
    if (launch_filter_or_ids(f->words, f->n_words, idb.as<uint32_t>(), n_ids, nullptr)) { mse_filter_free(f); return nullptr; }
    return filter_finish(f);
}

void mse_filter_free(mse_filter* f) {
    if (!f) return;
    if (f->words) (void)hipFree(f->words);
    if (f->ids) (void)hipFree(f->ids);
    delete f;
}
// The live rows of a graph as a filter: bit set where the row is not in the deleted map (and, with and_has_url and a has_url array, where
// has_url != 0).  Built on the device -- the NOT of the deleted words, filter.hip's and_flags_kernel in place, then the usual compaction
// -- under the graph's entry lock held shared, as mse_graph_compact reads it: a delete, restore or insert on another thread is wholly
// before or wholly after the snapshot.  The filter is a fresh object and immutable; later changes of the graph do not reach it.
mse_filter* mse_graph_live_filter(const mse_graph* g, int and_has_url) {
    if (!g) { fail("graph_live_filter: null graph"); return nullptr; }
    if (g->adj) {   // the filter belongs to the device the graph's arrays live on
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, g->adj) != hipSuccess) { (void)hipGetLastError(); fail("graph_live_filter: the graph's arrays are not device memory"); return nullptr; }
        if (hipSetDevice(at.device) != hipSuccess) { fail("graph_live_filter: hipSetDevice failed"); return nullptr; }
    }
    mse_filter* f = nullptr;
    {
        g->entry_lock.lock_shared();
        struct Hold { mse::SharedExclusive& l; ~Hold() { l.unlock_shared(); } } hold{g->entry_lock};
        f = filter_alloc(g->n);
        if (!f) return nullptr;
        bool ok = launch_filter_live(g->deleted, g->n, f->n_words, f->words, nullptr) == 0;
        if (ok && and_has_url && g->has_url) ok = launch_filter_and_flags(f->words, f->n_words, g->has_url, g->n, f->words, nullptr) == 0;
        if (ok && hipStreamSynchronize(nullptr) != hipSuccess) { ok = false; fail("graph_live_filter: the device pass failed"); }
        if (!ok) { mse_filter_free(f); return nullptr; }
    }
    return filter_finish(f);   // (reads the new bitmap only: the graph may change again)
}

size_t mse_filter_len(const mse_filter* f) { return f ? f->n_rows : 0; }
size_t mse_filter_count(const mse_filter* f) { return f ? f->count : 0; }

// ---- filters as values: set algebra, descriptor predicates, score thresholds, read-back (filter.hip) -----------------------------
// filter_finish with the id list sized by the count (count pass, read-back, allocation, write pass): what the creators below make holds
// count x 4 bytes of ids, not n_rows x 4.  `st`: the stream the bitmap was written on.  Frees f on failure.
static mse_filter* filter_finish_counted(mse_filter* f, hipStream_t st = nullptr) {
    DevBuf scratch;
    unsigned long long count = 0;
    bool ok = scratch.ensure(filter_compact_scratch_bytes(f->n_words) + 8) == 0;
    unsigned long long* count_dev = scratch.as<unsigned long long>();
    ok = ok && launch_filter_count(f->words, f->n_words, count_dev, scratch.as<char>() + 8, st) == 0;
    if (ok && (hipMemcpyAsync(&count, count_dev, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        ok = false; fail("filter: the count pass failed");
    }
    if (ok && hipMalloc((void**)&f->ids, std::max<size_t>((size_t)count, 1) * 4) != hipSuccess) { ok = false; fail("hipMalloc failed for the filter"); }
    ok = ok && launch_filter_write_ids(f->words, f->n_words, scratch.as<char>() + 8, f->ids, st) == 0;
    if (ok && hipStreamSynchronize(st) != hipSuccess) { ok = false; fail("filter: the compaction failed"); }
    if (!ok) { mse_filter_free(f); return nullptr; }
    f->count = (size_t)count;
    return f;
}

// the device `p` lives on becomes the thread's current device (as mse_graph_live_filter finds the graph's); 0, or -1 with the error set
static int enter_device_of(const void* p, const char* who) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(std::string(who) + ": not device memory");
    }
    if (hipSetDevice(at.device) != hipSuccess) return fail(std::string(who) + ": hipSetDevice failed");
    return 0;
}

// measurement hook (mse_filter_kernel_timing, for scripts/filter_ops_probe.py): while the switch is on, HIP events around the kernel
// that writes a new filter's bitmap -- not the count and write passes of filter_finish_counted, not from_scores' scan
static std::atomic<int> g_filter_timing{0};
static std::atomic<double> g_filter_kernel_ms{0.0};
struct FilterKernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    explicit FilterKernelTimer(hipStream_t stream) : st(stream) {
        if (!g_filter_timing.load()) return;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, st) != hipSuccess) drop();
    }
    void stop() {
        float ms = 0.0f;
        if (e0 && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
            g_filter_kernel_ms.store(ms);
    }
    void drop() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = nullptr;
        (void)hipGetLastError();
    }
    ~FilterKernelTimer() { drop(); }
};

int mse_filter_kernel_timing(int enable, double* last_ms) {
    if (last_ms) *last_ms = g_filter_kernel_ms.load();
    if (enable == 2) g_filter_kernel_ms.store(0.0);
    g_filter_timing.store(enable ? 1 : 0);
    return 0;
}

static mse_filter* filter_binary(const mse_filter* a, const mse_filter* b, int op, size_t n_rows) {
    if (hipSetDevice(a->device) != hipSuccess) { fail("filter: hipSetDevice failed"); return nullptr; }
    mse_filter* f = filter_alloc(n_rows);
    if (!f) return nullptr;
    FilterKernelTimer tm(nullptr);
    if (launch_filter_combine(a->words, a->n_words, b ? b->words : nullptr, b ? b->n_words : 0, op, n_rows, f->n_words, f->words, nullptr)) {
        mse_filter_free(f); return nullptr;
    }
    tm.stop();
    return filter_finish_counted(f);
}

mse_filter* mse_filter_combine(const mse_filter* a, const mse_filter* b, int op) {
    if (!a || !b) { fail("filter_combine: null filter"); return nullptr; }
    if (op < MSE_FILTER_AND || op > MSE_FILTER_ANDNOT) { fail("filter_combine: unknown op " + std::to_string(op)); return nullptr; }
    if (a->device != b->device) { fail("filter_combine: the filters were made on different devices"); return nullptr; }   // no silent copy
    return filter_binary(a, b, op, std::max(a->n_rows, b->n_rows));
}

mse_filter* mse_filter_not(const mse_filter* a, size_t n_rows) {
    if (!a) { fail("filter_not: null filter"); return nullptr; }
    if (n_rows == 0) n_rows = a->n_rows;
    if (n_rows < a->n_rows) {
        fail("filter_not: n_rows " + std::to_string(n_rows) + " is below the filter's " + std::to_string(a->n_rows) + " rows");
        return nullptr;
    }
    return filter_binary(a, nullptr, 4, n_rows);
}

mse_filter* mse_filter_from_descriptors(const mse_codes* c, const uint8_t* lo, const uint8_t* hi) {
    if (!c || !lo || !hi) { fail("filter_from_descriptors: null codes or bounds"); return nullptr; }
    if (!c->n_desc || !c->desc) { fail("filter_from_descriptors: the codes carry no descriptor bytes"); return nullptr; }
    if (c->n_desc > 8) { fail("filter_from_descriptors: at most 8 descriptor bytes per row"); return nullptr; }
    if (enter_device_of(c->desc, "filter_from_descriptors")) return nullptr;
    uint64_t lo8 = 0, hi8 = 0;
    for (size_t j = 0; j < c->n_desc; j++) { lo8 |= (uint64_t)lo[j] << (8 * j); hi8 |= (uint64_t)hi[j] << (8 * j); }
    mse_filter* f = filter_alloc(c->n);
    if (!f) return nullptr;
    FilterKernelTimer tm(nullptr);
    if (launch_filter_desc_range(c->desc, (int)c->n_desc, c->n, lo8, hi8, f->n_words, f->words, nullptr)) { mse_filter_free(f); return nullptr; }
    tm.stop();
    return filter_finish_counted(f);
}

mse_filter* mse_filter_from_scores(mse_searcher* s, const uint16_t* query, int64_t threshold, const mse_filter* within) {
    if (!s || !s->base) { fail("filter_from_scores: null searcher"); return nullptr; }
    if (!query) { fail("filter_from_scores: null query"); return nullptr; }
    const mse_base* b = s->base;
    if (within && check_filter(b, within)) return nullptr;
    if (hipSetDevice(b->device) != hipSuccess) { fail("filter_from_scores: hipSetDevice failed"); return nullptr; }
    mse_filter* f = filter_alloc(b->n);
    if (!f) return nullptr;
    const size_t d = b->d;
    bool ok = true;
    if (b->n) {   // the one query staged and scored as mse_bruteforce_scores_f16 does it, then the threshold pass over s->scores
        ok = s->q_stage.ensure(8 * d * 2) == 0 && s->scores.ensure(b->n * 8) == 0;
        if (ok && (hipMemsetAsync(s->q_stage.p, 0, 8 * d * 2, s->stream) != hipSuccess ||
                   hipMemcpyAsync(s->q_stage.p, query, d * 2, hipMemcpyHostToDevice, s->stream) != hipSuccess)) {
            ok = false; fail("filter_from_scores: staging the query failed");
        }
        ok = ok && launch_scan_exact(b->dev, b->n, (int)d, s->q_stage.p, 1, false, s->scores.as<int64_t>(), b->n, nullptr, s->n_cu, s->stream) == 0;
        FilterKernelTimer tm(s->stream);
        ok = ok && launch_filter_score_threshold(s->scores.as<int64_t>(), b->n, threshold, within ? within->words : nullptr,
                                                 within ? within->n_words : 0, f->n_words, f->words, s->stream) == 0;
        if (ok) tm.stop();
    }
    if (!ok) { (void)hipStreamSynchronize(s->stream); mse_filter_free(f); return nullptr; }
    return filter_finish_counted(f, s->stream);
}

mse_filter* mse_filter_from_bits_dev(const void* bits_dev, size_t n_rows) {
    if (!bits_dev && n_rows) { fail("filter_from_bits_dev: null bitmap"); return nullptr; }
    if (n_rows && enter_device_of(bits_dev, "filter_from_bits_dev")) return nullptr;
    mse_filter* f = filter_alloc(n_rows);
    if (!f) return nullptr;
    FilterKernelTimer tm(nullptr);
    bool ok = hipMemsetAsync(f->words, 0, std::max<size_t>(f->n_words, 1) * 4, nullptr) == hipSuccess;
    if (ok && n_rows) ok = hipMemcpyAsync(f->words, bits_dev, (n_rows + 7) / 8, hipMemcpyDeviceToDevice, nullptr) == hipSuccess;
    if (!ok) { mse_filter_free(f); fail("filter_from_bits_dev: the device copy failed"); return nullptr; }
    if (launch_filter_mask_tail(f->words, n_rows, nullptr)) { mse_filter_free(f); return nullptr; }
    tm.stop();
    return filter_finish_counted(f);
}

int mse_filter_to_bits(const mse_filter* f, uint8_t* bits) {
    if (!f) return fail("filter_to_bits: null filter");
    if (!bits) return fail("filter_to_bits: null buffer");
    if (f->n_rows == 0) return 0;
    if (hipMemcpy(bits, f->words, (f->n_rows + 7) / 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("filter_to_bits: the read-back failed");
    return 0;
}

int mse_filter_read_ids(const mse_filter* f, size_t first, size_t n, uint32_t* out) {
    if (!f) return fail("filter_read_ids: null filter");
    if (first > f->count || n > f->count - first)
        return fail("filter_read_ids: [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") is past the filter's " +
                    std::to_string(f->count) + " allowed rows");
    if (n == 0) return 0;
    if (!out) return fail("filter_read_ids: null buffer");
    if (hipMemcpy(out, f->ids + first, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("filter_read_ids: the read-back failed");
    return 0;
}

// ---- a filter over GLOBAL rows cut into filters over LOCAL rows, and back (filter.hip slice_words_kernel / place_words_kernel) ----------
static int resolve_filter_device(int device, int own, const char* who) {
    if (device < 0) return own;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) { fail(std::string(who) + ": device ordinal out of range"); return -1; }
    return device;
}

mse_filter* mse_filter_slice(const mse_filter* src, uint64_t first_row, size_t n_rows, int device) {
    if (!src) { fail("filter_slice: null filter"); return nullptr; }
    if (n_rows == 0) { fail("filter_slice: n_rows must be positive"); return nullptr; }
    if (first_row > 0xFFFFFFFEull) { fail("filter_slice: row ids are u32: first_row is too large"); return nullptr; }
    const int dev = resolve_filter_device(device, src->device, "filter_slice");
    if (dev < 0) return nullptr;
    DeviceScope scope(dev);
    if (!scope.ok) { fail("filter_slice: hipSetDevice failed"); return nullptr; }
    mse_filter* f = filter_alloc(n_rows);
    if (!f) return nullptr;
    const uint32_t* in = src->words;
    size_t in_words = src->n_words, in_rows = src->n_rows;
    uint64_t first = first_row;
    DevBuf range;   // another device: the word range the slice reads comes over by ONE peer copy and is sliced here
    if (dev != src->device) {
        const size_t w0 = std::min<size_t>((size_t)(first_row >> 5), src->n_words);
        const size_t nw = std::min<size_t>(src->n_words - w0, (n_rows + 31) / 32 + 1);
        if (range.ensure(std::max<size_t>(nw, 1) * 4)) { mse_filter_free(f); return nullptr; }
        if (nw && hipMemcpyPeer(range.p, dev, src->words + w0, src->device, nw * 4) != hipSuccess) {
            (void)hipGetLastError();
            mse_filter_free(f); fail("filter_slice: the peer copy failed"); return nullptr;
        }
        in = range.as<uint32_t>(); in_words = nw;
        in_rows = src->n_rows > w0 * 32 ? src->n_rows - w0 * 32 : 0;
        first = first_row - (uint64_t)w0 * 32;
    }
    FilterKernelTimer tm(nullptr);
    if (launch_filter_slice(in, in_words, in_rows, first, n_rows, f->n_words, f->words, nullptr)) { mse_filter_free(f); return nullptr; }
    tm.stop();
    return filter_finish_counted(f);   // (blocks: `range` is free to go afterwards)
}

mse_filter* mse_filter_concat(const mse_filter* const* parts, const uint64_t* first_rows, size_t n_parts, size_t n_rows, int device) {
    if (n_parts && (!parts || !first_rows)) { fail("filter_concat: null argument"); return nullptr; }
    if (n_rows == 0) { fail("filter_concat: n_rows must be positive"); return nullptr; }
    std::vector<std::pair<uint64_t, uint64_t>> spans;   // [first, end) of the parts that hold rows
    for (size_t i = 0; i < n_parts; i++) {
        if (!parts[i]) { fail("filter_concat: null part " + std::to_string(i)); return nullptr; }
        const uint64_t len = parts[i]->n_rows;
        if (first_rows[i] > n_rows || len > n_rows - first_rows[i]) {
            fail("filter_concat: part " + std::to_string(i) + " reaches past the result's " + std::to_string(n_rows) + " rows");
            return nullptr;
        }
        if (len) spans.emplace_back(first_rows[i], first_rows[i] + len);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        if (spans[i].first < spans[i - 1].second) { fail("filter_concat: parts overlap at row " + std::to_string(spans[i].first)); return nullptr; }
    int own = 0;
    if (n_parts) own = parts[0]->device;
    else if (hipGetDevice(&own) != hipSuccess) own = 0;
    const int dev = resolve_filter_device(device, own, "filter_concat");
    if (dev < 0) return nullptr;
    DeviceScope scope(dev);
    if (!scope.ok) { fail("filter_concat: hipSetDevice failed"); return nullptr; }
    mse_filter* f = filter_alloc(n_rows);
    if (!f) return nullptr;
    // all on the null stream, one launch per part: parts that share a boundary word meet in launch order
    FilterKernelTimer tm(nullptr);
    bool ok = hipMemsetAsync(f->words, 0, std::max<size_t>(f->n_words, 1) * 4, nullptr) == hipSuccess;
    if (!ok) fail("filter_concat: clearing the bitmap failed");
    std::vector<DevBuf> staged(n_parts);   // parts of another device: their words come over by one peer copy each
    for (size_t i = 0; ok && i < n_parts; i++) {
        const mse_filter* p = parts[i];
        if (p->n_rows == 0) continue;
        const uint32_t* words = p->words;
        if (p->device != dev) {
            const size_t nw = (p->n_rows + 31) / 32;
            ok = staged[i].ensure(nw * 4) == 0;
            if (ok && hipMemcpyPeer(staged[i].p, dev, p->words, p->device, nw * 4) != hipSuccess) {
                (void)hipGetLastError();
                ok = false; fail("filter_concat: the peer copy failed");
            }
            words = staged[i].as<uint32_t>();
        }
        ok = ok && launch_filter_place(words, p->n_rows, first_rows[i], n_rows, f->words, nullptr) == 0;
    }
    if (!ok) { (void)hipStreamSynchronize(nullptr); mse_filter_free(f); return nullptr; }
    tm.stop();
    return filter_finish_counted(f);
}

}  // extern "C"
