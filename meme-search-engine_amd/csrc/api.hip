// C ABI (include/mse.h): runtime, base vectors, searcher; the selection tournament (descend) and its test hook.
#include <cstdlib>
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <map>
#include <mutex>
#include <new>

namespace mse {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(const std::string& msg) {
    g_last_error = msg;
    return -1;
}

int ensure_dyn_lds(const void* kernel, int bytes) {
    int dev = 0;
    MSE_HIP_TRY(hipGetDevice(&dev));
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, int> granted;
    std::lock_guard<std::mutex> lk(mu);
    int& have = granted[{kernel, dev}];
    if (have >= bytes) return 0;
    MSE_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
    return 0;
}

int DevBuf::ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    size_t want = (bytes + 255) & ~(size_t)255;
    MSE_HIP_TRY(hipMalloc(&p, want));
    cap = want;
    return 0;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}
int PinBuf::ensure(size_t bytes, size_t floor) {
    if (bytes <= cap) return 0;
    release();
    const size_t want = std::max(2 * bytes, floor);
    MSE_HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return 0;
}
void PinBuf::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

int device_cu_count() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    return n;
}

constexpr size_t DENSE_MAX = 16384;  // a level this small is selected from directly

mse_searcher* scratch_searcher_new() {
    mse_searcher* s = new (std::nothrow) mse_searcher();
    if (!s) { fail("out of host memory"); return nullptr; }
    s->n_cu = device_cu_count();
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        delete s; fail("hipStreamCreate failed"); return nullptr;
    }
    s->own_stream = true;
    return s;
}

// Tournament descent (topk.hip header).  Leaves the ids of the k best level-0 entries per query in
// *sel_out ([nq][k], best first) and, when keys_out != nullptr, their raw keys in keys_out.
int descend(mse_searcher* s, const LevelRef& l0, int nq, int k, uint32_t** sel_out, void* keys_out) {
    hipStream_t st = s->stream;
    std::vector<LevelRef> lv;
    lv.push_back(l0);
    int li = 0;
    while (lv.back().n > DENSE_MAX) {
        const LevelRef cur = lv.back();
        const size_t n_out = (cur.n + TOPK_FANOUT - 1) / TOPK_FANOUT;
        const bool k64 = (cur.kind == KEY_I64 || cur.kind == KEY_U64);
        if (li >= 6) return fail("descend: too many levels");
        if (s->levels[li].ensure((size_t)nq * n_out * (k64 ? 8 : 4))) return -1;
        if (cur.group_major) {
            if (launch_reduce_max_gq(reinterpret_cast<const float*>(cur.ptr), cur.nq_pad, cur.n,
                                     s->levels[li].as<uint32_t>(), n_out, n_out, nq, st)) return -1;
        } else {
            if (launch_reduce_max(cur.kind, cur.ptr, cur.q_stride, cur.n, s->levels[li].p, n_out, n_out, nq, st, cur.e_stride))
                return -1;
        }
        lv.push_back(LevelRef{k64 ? KEY_U64 : KEY_U32, s->levels[li].p, n_out, 1, n_out, false, 0});
        li++;
    }
    if (s->sel_a.ensure((size_t)nq * k * 4) || s->sel_b.ensure((size_t)nq * k * 4) || s->thr.ensure((size_t)nq * 16)) return -1;
    uint32_t* cur_sel = s->sel_a.as<uint32_t>();
    uint32_t* nxt_sel = s->sel_b.as<uint32_t>();
    // each level hands the score key of its k-th best entry down as a floor: every one of the k best parents has a child with
    // exactly its key, so at least k children reach the floor and everything below it can be skipped unread by the radix passes
    unsigned long long* kth_cur = s->thr.as<unsigned long long>();
    unsigned long long* kth_nxt = kth_cur + nq;
    const int top = (int)lv.size() - 1;
    {
        SelectArgs a{};
        const LevelRef& L = lv[top];
        a.kind = L.kind; a.in = L.ptr; a.in_stride = L.q_stride; a.n_in = L.n;
        a.k = k; a.out_ids = cur_sel; a.out_keys = top == 0 ? keys_out : nullptr; a.out_stride = k; a.nq = nq;
        a.kth_hi_out = kth_cur;
        if (launch_select_strided(a, L.e_stride, st)) return -1;
    }
    for (int l = top - 1; l >= 0; l--) {
        SelectArgs a{};
        const LevelRef& L = lv[l];
        a.kind = L.kind; a.in = L.ptr; a.in_stride = L.q_stride; a.n_in = L.n;
        a.parents = cur_sel; a.par_stride = k; a.n_par = k; a.fanout = TOPK_FANOUT;
        a.k = k; a.out_ids = nxt_sel; a.out_keys = l == 0 ? keys_out : nullptr; a.out_stride = k; a.nq = nq;
        a.floor_hi = kth_cur; a.kth_hi_out = kth_nxt;
        if (launch_select_strided(a, L.e_stride, st)) return -1;
        std::swap(cur_sel, nxt_sel);
        std::swap(kth_cur, kth_nxt);
    }
    s->last_kth = kth_cur;
    *sel_out = cur_sel;
    return 0;
}

size_t visited_budget_bytes() {
    const char* e = getenv("MSE_VISITED_BUDGET_KB");
    if (e) return (size_t)atoll(e) * 1024;
    // half of what is free right now, between 256 MiB and 64 GiB (an index that fills the HBM leaves little; a small one leaves
    // room for every query of a batch at once)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (size_t)4 << 30;
    size_t b = free_b / 2;
    if (b < ((size_t)256 << 20)) b = (size_t)256 << 20;
    if (b > ((size_t)64 << 30)) b = (size_t)64 << 30;
    return b;
}

}  // namespace mse

using namespace mse;

extern "C" {

const char* mse_last_error(void) { return g_last_error.c_str(); }
const char* mse_version(void) { return "mse-hip 0.1 (gfx950)"; }

int mse_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int mse_set_device(int ordinal) {
    MSE_HIP_TRY(hipSetDevice(ordinal));
    return 0;
}
int mse_device_synchronize(void) {
    MSE_HIP_TRY(hipDeviceSynchronize());
    return 0;
}
int mse_device_mem_info(size_t* free_bytes, size_t* total_bytes) {
    size_t f = 0, t = 0;
    MSE_HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

int64_t mse_scale_dot_f32(float x) { return scale_dot_result(x); }
int64_t mse_scale_dot_f64(double x) { return scale_dot_result_f64(x); }

// ---- base ------------------------------------------------------------------------------------
static mse_base* base_alloc(size_t n, size_t d, bool owned) {
    if (d == 0 || d % 64 != 0 || d > (size_t)D_MAX) {
        fail("vector width must be a positive multiple of 64 (fast_dot asserts len % 64 == 0)");
        return nullptr;
    }
    if (n > 0xFFFFFFFEull) {
        fail("row ids are u32: too many rows");
        return nullptr;
    }
    mse_base* b = new (std::nothrow) mse_base();
    if (!b) { fail("out of host memory"); return nullptr; }
    b->n = n; b->d = d; b->owned = owned; b->n_cu = device_cu_count();
    if (hipGetDevice(&b->device) != hipSuccess) b->device = 0;
    return b;
}
mse_base* mse_base_from_host(const uint16_t* data, size_t n_rows, size_t d) {
    mse_base* b = base_alloc(n_rows, d, true);
    if (!b) return nullptr;
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(n_rows * d * 2, 256);
    if (hipMalloc(&p, bytes) != hipSuccess) { delete b; fail("hipMalloc failed for base vectors"); return nullptr; }
    if (n_rows && hipMemcpy(p, data, n_rows * d * 2, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p); delete b; fail("hipMemcpy failed for base vectors"); return nullptr;
    }
    b->dev = reinterpret_cast<const uint16_t*>(p);
    return b;
}
mse_base* mse_base_wrap_device(const void* data_dev, size_t n_rows, size_t d) {
    mse_base* b = base_alloc(n_rows, d, false);
    if (!b) return nullptr;
    b->dev = reinterpret_cast<const uint16_t*>(data_dev);
    // the device that holds the rows, not the one that happens to be current on the calling thread: worker threads made for this
    // base (coalescer, shard group) select b->device
    hipPointerAttribute_t at{};
    if (data_dev && hipPointerGetAttributes(&at, data_dev) == hipSuccess) {
        if (at.type == hipMemoryTypeDevice) b->device = at.device;
    } else {
        (void)hipGetLastError();
    }
    return b;
}
mse_base* mse_base_generate(uint32_t seed, uint64_t first_row, size_t n_rows, size_t d) {
    mse_base* b = base_alloc(n_rows, d, true);
    if (!b) return nullptr;
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(n_rows * d * 2, 256);
    if (hipMalloc(&p, bytes) != hipSuccess) { delete b; fail("hipMalloc failed for base vectors"); return nullptr; }
    b->dev = reinterpret_cast<const uint16_t*>(p);
    if (launch_generate_rows(reinterpret_cast<uint16_t*>(p), seed, first_row, n_rows, (int)d, nullptr) ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(p); delete b; if (g_last_error.empty()) fail("row generation failed"); return nullptr;
    }
    return b;
}
mse_base* mse_base_select(const mse_base* b, const mse_filter* keep) {
    if (!b) { fail("base_select: null base"); return nullptr; }
    if (check_filter(b, keep)) return nullptr;
    if (hipSetDevice(b->device) != hipSuccess) { fail("base_select: hipSetDevice failed"); return nullptr; }
    mse_base* out = base_alloc(keep->count, b->d, true);
    if (!out) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(keep->count * b->d * 2, 256)) != hipSuccess) { delete out; fail("hipMalloc failed for base vectors"); return nullptr; }
    out->dev = reinterpret_cast<const uint16_t*>(p);
    // 16-byte pieces when the source allows them (a wrapped base may start anywhere), 2-byte elements otherwise
    const bool vec16 = reinterpret_cast<uintptr_t>(b->dev) % 16 == 0;
    const int rc = vec16 ? launch_join_select_rows(b->dev, b->d * 2, keep->ids, keep->count, p, b->n_cu, nullptr)
                         : launch_gather_rows_f16(b->dev, keep->ids, keep->count, (int)b->d, reinterpret_cast<uint16_t*>(p), nullptr);
    if (rc || hipStreamSynchronize(nullptr) != hipSuccess) {
        mse_base_free(out); if (!rc) fail("base_select: the row gather failed"); return nullptr;
    }
    return out;
}
void mse_base_free(mse_base* b) {
    if (!b) return;
    if (b->disp) mse_dispatcher_free(b->disp);   // joins its worker; no search may be in flight (as for the rows themselves)
    if (b->owned && b->dev) (void)hipFree(const_cast<uint16_t*>(b->dev));
    if (b->norm_bits_dev) (void)hipFree(b->norm_bits_dev);
    delete b;
}
int mse_base_rows_changed(mse_base* b) {
    if (!b) return fail("null base");
    std::lock_guard<std::mutex> g(b->norm_mu);
    b->norm_ready = false;
    return 0;
}
size_t mse_base_len(const mse_base* b) { return b ? b->n : 0; }
size_t mse_base_dim(const mse_base* b) { return b ? b->d : 0; }
const void* mse_base_device_ptr(const mse_base* b) { return b ? b->dev : nullptr; }
int mse_base_read_rows(const mse_base* b, size_t first_row, size_t n_rows, uint16_t* out) {
    if (!b) return fail("null base");
    if (first_row + n_rows > b->n) return fail("row range out of bounds");
    if (n_rows == 0) return 0;
    MSE_HIP_TRY(hipMemcpy(out, b->dev + first_row * b->d, n_rows * b->d * 2, hipMemcpyDeviceToHost));
    return 0;
}

int mse_fast_dot_f16(const uint16_t* x, const uint16_t* y, size_t n, int64_t* out) {
    if (n == 0 || n % 64 != 0 || n > (size_t)D_MAX) return fail("fast_dot: length must be a positive multiple of 64");
    DevBuf buf;
    if (buf.ensure(n * 4 + 64)) return -1;
    char* p = buf.as<char>();
    uint32_t zero = 0;
    MSE_HIP_TRY(hipMemcpy(p, x, n * 2, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(p + n * 2, y, n * 2, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(p + n * 4, &zero, 4, hipMemcpyHostToDevice));
    if (launch_score_rows(reinterpret_cast<const uint16_t*>(p + n * 2), 1, (int)n, p, false,
                          reinterpret_cast<const uint32_t*>(p + n * 4), 1, 1, reinterpret_cast<int64_t*>(p + n * 4 + 8),
                          nullptr, nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, p + n * 4 + 8, 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- searcher --------------------------------------------------------------------------------
mse_searcher* mse_searcher_new(const mse_base* b) {
    if (!b) { fail("null base"); return nullptr; }
    mse_searcher* s = new (std::nothrow) mse_searcher();
    if (!s) { fail("out of host memory"); return nullptr; }
    s->base = b;
    s->n_cu = b->n_cu;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        delete s; fail("hipStreamCreate failed"); return nullptr;
    }
    s->own_stream = true;
    return s;
}
void mse_searcher_free(mse_searcher* s) {
    if (!s) return;
    if (s->own_stream && s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    for (hipEvent_t e : s->join.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->ev_pool) (void)hipEventDestroy(e);
    if (s->ev_wait) (void)hipEventDestroy(s->ev_wait);
    for (hipEvent_t e : s->grp_ev)
        if (e) (void)hipEventDestroy(e);
    if (s->bev0) (void)hipEventDestroy(s->bev0);
    if (s->bev1) (void)hipEventDestroy(s->bev1);
    delete s;
}
int mse_searcher_set_stream(mse_searcher* s, void* hip_stream) {
    if (!s) return fail("null searcher");
    if (s->own_stream && s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    s->stream = reinterpret_cast<hipStream_t>(hip_stream);
    s->own_stream = false;
    return 0;
}
void* mse_searcher_stream(const mse_searcher* s) { return s ? (void*)s->stream : nullptr; }
int mse_searcher_scan_timing(mse_searcher* s, int enable, double* total_ms, uint64_t* launches) {
    if (!s) return fail("null searcher");
    if (total_ms) *total_ms = s->scan_ms_total;
    if (launches) *launches = s->scan_launches;
    if (enable && !s->ev0) {
        MSE_HIP_TRY(hipEventCreate(&s->ev0));
        MSE_HIP_TRY(hipEventCreate(&s->ev1));
    }
    if (enable == 2) { s->scan_ms_total = 0.0; s->scan_launches = 0; }
    s->timing = enable != 0;
    return 0;
}
int mse_searcher_last_stats(const mse_searcher* s, uint32_t* n_widened, uint32_t* max_groups) {
    if (!s) return fail("null searcher");
    if (n_widened) *n_widened = s->last_widened;
    if (max_groups) *max_groups = s->last_max_groups;
    return 0;
}
int mse_searcher_set_sparse_maxima(mse_searcher* s, int mode, uint32_t stride, uint32_t capacity) {
    if (!s) return fail("null searcher");
    if (mode < 0 || mode > 2) return fail("sparse maxima: mode 0 (auto), 1 (off) or 2 (forced)");
    if (stride && (stride < 3 || stride > 1025 || ((stride - 1) & (stride - 2)) != 0))
        return fail("sparse maxima: the sample stride must be 2^j + 1, 3 .. 1025");
    if (capacity > (1u << 20)) return fail("sparse maxima: at most 2^20 survivors per query");
    s->sparse_mode = mode;
    if (stride) s->sparse_stride = stride;
    if (capacity) s->sparse_cap = capacity;
    return 0;
}
int mse_searcher_sparse_stats(const mse_searcher* s, uint32_t* passes, uint32_t* fallbacks, uint32_t* longest_list) {
    if (!s) return fail("null searcher");
    if (passes) *passes = s->last_sparse_passes;
    if (fallbacks) *fallbacks = s->last_sparse_fallbacks;
    if (longest_list) *longest_list = s->last_sparse_max_list;
    return 0;
}

size_t mse_queries_per_pass_max(size_t d) { return d && d % 64 == 0 ? (size_t)mfma_query_tile((int)d) : 0; }

// test hook: descend() over keys the caller supplies, so that the tournament and the radix select can be checked on keys no search
// produces (tests/test_gpu_topk_select.py).  The level-0 forms are the callers': query-major (exact_pass, the PQ gather), element-strided
// (the batched PQ scan's u32 group maxima), group-major float (the MFMA rounds).  descend() hands keys_out to the level-0 select on
// every path -- the only select when n <= DENSE_MAX, the last of the descent otherwise -- so the keys come back for every kind and
// layout accepted here; everything else is refused.
int mse_debug_select_topk(mse_searcher* s, int kind, int layout, const void* keys, size_t n, size_t nq, size_t nq_pad, size_t k,
                          uint32_t* ids_out, void* keys_out, uint64_t* kth_out) {
    if (!s) return fail("null searcher");
    if (!keys || !ids_out || !keys_out || !kth_out) return fail("select_topk: null array");
    if (k == 0 || k > (size_t)TOPK_KMAX) return fail("select_topk: k must be 1.." + std::to_string(TOPK_KMAX));
    if (n == 0 || n > 0xFFFFFFFEull) return fail("select_topk: 1..2^32-2 keys per query (ids are u32)");
    if (nq == 0 || nq > 65536) return fail("select_topk: 1..65536 queries");
    if (kind != KEY_I64 && kind != KEY_F32 && kind != KEY_U32) return fail("select_topk: kind must be 0 (i64), 1 (f32) or 3 (u32)");
    if (layout < 0 || layout > 2 || (layout == 2 && kind != KEY_F32)) return fail("select_topk: layout 0, 1, or 2 with f32 keys only");
    if (layout == 0) nq_pad = nq;
    if (nq_pad < nq || nq_pad > 65536) return fail("select_topk: nq_pad must be nq..65536");
    const size_t es = kind == KEY_I64 ? 8 : 4;
    DevBuf& in = layout == 0 ? s->scores : s->gmax;
    if (in.ensure(n * nq_pad * es) || s->sel_keys.ensure(nq * k * es)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(in.p, keys, n * nq_pad * es, hipMemcpyHostToDevice, s->stream));
    const LevelRef l0 = layout == 0   ? LevelRef{(KeyKind)kind, in.p, n, 1, n, false, 0}
                        : layout == 1 ? LevelRef{(KeyKind)kind, in.p, 1, nq_pad, n, false, 0}
                                      : LevelRef{KEY_F32, in.p, 1, nq_pad, n, true, (int)nq_pad};
    uint32_t* sel = nullptr;
    s->last_kth = nullptr;
    if (descend(s, l0, (int)nq, (int)k, &sel, s->sel_keys.p)) return -1;
    if (!sel || !s->last_kth) return fail("select_topk: descend() left no selection behind");
    MSE_HIP_TRY(hipMemcpyAsync(ids_out, sel, nq * k * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(keys_out, s->sel_keys.p, nq * k * es, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(kth_out, s->last_kth, nq * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

int mse_merge_topk_dev(mse_searcher* s, const void* gathered_scores_dev, const void* gathered_ids_dev,
                       size_t n_shards, size_t nq, size_t k, void* out_scores_dev, void* out_ids_dev) {
    if (!s) return fail("null searcher");
    if (nq == 0 || k == 0 || n_shards == 0) return 0;
    if (k > (size_t)TOPK_KMAX) return fail("k too large");
    if (s->misc.ensure(nq * k * 4) || s->sel_keys.ensure(nq * k * 8)) return -1;
    SelectArgs a{};
    a.kind = KEY_I64;
    a.list_ids = reinterpret_cast<const uint32_t*>(gathered_ids_dev);
    a.list_keys = gathered_scores_dev;
    a.list_stride = k;                 // query q starts k records into each shard block
    a.list_chunk = k;
    a.list_chunk_stride = nq * k;      // next shard
    a.n_list = n_shards * k;
    a.k = (int)k; a.out_ids = s->misc.as<uint32_t>(); a.out_keys = s->sel_keys.p; a.out_stride = k; a.nq = (int)nq;
    if (launch_select(a, s->stream)) return -1;
    return launch_finalize(s->misc.as<uint32_t>(), s->sel_keys.as<int64_t>(), k, (int)k, (int)nq, 0,
                           reinterpret_cast<int64_t*>(out_scores_dev), reinterpret_cast<uint32_t*>(out_ids_dev), k,
                           nullptr, 0, 0, 0, nullptr, nullptr, s->stream);
}

}  // extern "C"
