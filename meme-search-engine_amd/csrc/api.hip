// C ABI (include/mse.h): runtime, base vectors, searcher, brute-force search, flat index.
#include <cstdlib>
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
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

int ensure_base_norm(const mse_base* b, hipStream_t st) {
    std::lock_guard<std::mutex> g(b->norm_mu);
    if (b->norm_ready) return 0;
    if (!b->norm_bits_dev) MSE_HIP_TRY(hipMalloc((void**)&b->norm_bits_dev, 12));   // [max norm, max subnormal mass of a row, max |x_i|]
    MSE_HIP_TRY(hipMemsetAsync(b->norm_bits_dev, 0, 12, st));
    if (launch_row_norm_max(b->dev, b->n, (int)b->d, b->norm_bits_dev, st)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(st));
    b->norm_ready = true;
    return 0;
}

// exact mode, one pass of <= 8 queries already staged (padded) in s->q_stage.  With a filter (non-empty, no longer than the base):
// the filter's allowed rows only, scanned through its ascending id list; level 0 then holds list positions, so an excluded row is
// absent -- not merely low: an allowed row whose score saturates to INT64_MIN still ranks -- and (score desc, position asc) is
// (score desc, id asc).  The selected positions are mapped back to row ids before the finish.
static int exact_pass(mse_searcher* s, int nq_pass, int k, uint64_t id_offset, int64_t* out_scores, uint32_t* out_ids,
                      size_t out_stride, const mse_filter* f = nullptr) {
    return exact_pass_list(s, nq_pass, k, id_offset, out_scores, out_ids, out_stride, f ? f->ids : nullptr, f ? f->count : s->base->n, nullptr);
}

// The pass itself: rows ids[0 .. n) (ascending; null = rows 0 .. n), and -- the filtered graph search's LIST regime -- the descriptor
// bias of every listed row added to its score BEFORE the selection (bias: descriptors, their count, the pass's scales on the device).
int exact_pass_list(mse_searcher* s, int nq_pass, int k, uint64_t id_offset, int64_t* out_scores, uint32_t* out_ids, size_t out_stride,
                    const uint32_t* ids, size_t n, const ListBias* bias) {
    const mse_base* b = s->base;
    if (s->scores.ensure((size_t)nq_pass * n * 8)) return -1;
    if (launch_scan_exact(b->dev, n, (int)b->d, s->q_stage.p, nq_pass, false, s->scores.as<int64_t>(), n, nullptr,
                          s->n_cu, s->stream, ids)) return -1;
    if (bias && launch_list_bias(ids, n, bias->desc, bias->n_desc, bias->scales_dev, nq_pass, s->scores.as<int64_t>(), n, s->stream)) return -1;
    if (s->sel_keys.ensure((size_t)nq_pass * k * 8)) return -1;
    uint32_t* sel = nullptr;
    LevelRef l0{KEY_I64, s->scores.p, n, 1, n, false, 0};
    if (descend(s, l0, nq_pass, k, &sel, s->sel_keys.p)) return -1;
    if (ids && launch_map_positions(sel, (size_t)nq_pass * k, ids, s->stream)) return -1;
    return launch_finalize(sel, s->sel_keys.as<int64_t>(), k, k, nq_pass, id_offset, out_scores, out_ids, out_stride,
                           nullptr, 0, 0, 0, nullptr, nullptr, s->stream);
}

// How many queries one call of mfma_pass may take: one pass over the rows (mfma_query_tile) for a large base; for a SMALL base -- group
// maxima of all queries within 256 MiB -- up to 8192, scanned pass by pass into one wide array of group maxima and finished by ONE
// tournament / re-score / certificate over all of them.  The fixed cost of a pass (a dozen small launches and a host synchronisation
// for the margins) is what a small base pays for: 4096 queries against a 4096-row entry table (the request path's entry step,
// beam_search.hip) took 13 passes x 0.28 ms.
static size_t mfma_call_tile(const mse_base* b, size_t k) {
    const size_t tile = (size_t)mfma_query_tile((int)b->d);
    const size_t n_groups = (b->n + GROUP_ROWS - 1) / GROUP_ROWS;
    size_t fit = ((size_t)256 << 20) / (std::max<size_t>(n_groups, 1) * 4) / tile * tile;
    // the first round re-scores (k + 8) groups of 32 or 64 rows (mfma_pass) per query: ids + scores of all queries within 1 GiB
    const size_t per_query = std::min<size_t>(std::max<size_t>(k + 8, 16), TOPK_KMAX) * 64 * 12;
    fit = std::min(fit, ((size_t)1 << 30) / per_query / tile * tile);
    if (fit > 8192 / tile * tile) fit = 8192 / tile * tile;
    return std::max(fit, tile);
}

// MFMA mode for up to mfma_call_tile(base) queries (device pointer to [nq][d] f16, contiguous).  With a filter: the scan's group
// maxima are over allowed rows only (-FLT_MAX for a group without one), candidate expansion drops excluded rows, and the exact
// fallback is the filtered exact pass; the certificate is unchanged (every allowed row outside the chosen groups is at most its
// group's masked maximum, and the largest row norm still bounds eps).
// Rows per group maximum (gr): 64 when every pass of the call is a 320-query pass, whose waves own 64 rows each (mfma_group_rows),
// else 32.  The certificate does not care -- every row outside the chosen groups is at most its group's maximum, whatever a group is --
// and the kg0 groups re-scored per query are then twice as many rows.
// The queries are read where the caller has them: the scan's pack kernel writes the padding of the last pass as zeros, and the norms,
// the re-score and the widening only ever touch the nq_pass real rows.
// Thresholded group maxima (`sparse`, the 320-query unmasked pass with 64-row groups only).  The dense array of group
// maxima is 4 B x 320 per 64 rows written by the scan and read back once by the tournament, and all but a few hundred entries per query
// are never looked at again.  Instead: launch A scans every S-th 256-row tile (the sample) with the dense epilogue into a small array;
// the tournament over it gives G_k, the k-th best sample group maximum of each query; tau_q = the float below G_k - 3 eps_q (topk.hip
// sparse_tau_kernel has the argument: no row of a group whose maximum is <= tau_q can be in the exact top k, not even as a tie);
// launch B scans the other tiles and appends (group, maximum) to the query's list only where maximum > tau_q.  The round then picks
// its kg best groups from the list, and the certificate's bound is max(last chosen key, tau_q): what is not on the list is <= tau_q.
// Widening takes more of the same list; a list used up leaves tau_q, which certifies by construction.  A query whose survivors exceed
// the list capacity (an unrepresentative sample, heavily duplicated rows) sets *overflow: the caller runs the pass again the dense way.
struct SparsePlan {
    uint32_t stride = 0, cap = 0, shift = 0;
    size_t n_a = 0, n_b = 0, n_sg = 0;   // sample tiles, other tiles, sample groups that exist
};
static bool sparse_plan(const mse_searcher* s, int nq_pass, int k, const mse_filter* f, SparsePlan* p) {
    const mse_base* b = s->base;
    const int d = (int)b->d;
    if (s->sparse_mode == 1 || f || mfma_query_tile(d) != 320 || nq_pass > 320 || mfma_pad(nq_pass, d) != 320 || mfma_group_rows(320) != 64) return false;
    const uint32_t S = s->sparse_stride;
    const size_t n_tiles = (b->n + 255) / 256, n_groups = (b->n + 63) / 64;
    p->stride = S; p->cap = s->sparse_cap;
    p->shift = 0;
    while ((1u << p->shift) < S - 1) p->shift++;
    p->n_a = (n_tiles + S - 1) / S;
    p->n_b = n_tiles - p->n_a;
    p->n_sg = (p->n_a - 1) * 4 + std::min<size_t>(4, n_groups - (p->n_a - 1) * (size_t)S * 4);
    // what correctness needs: G_k must exist, i.e. the sample holds k groups
    if (n_tiles < 2 || p->n_sg < (size_t)k) return false;
    if (s->sparse_mode == 2) return true;
    // auto: each launch keeps every CU busy for at least eight tiles (a second launch costs the drain and fill of the persistent grid,
    // about one tile per CU); the sample holds four times the groups a round re-scores, so that G_k is a typical k-th maximum; and the
    // survivors expected of random rows, about k * S per query, fit the list four times over
    const size_t kg0 = std::min<size_t>(std::max(k + 8, 16), TOPK_KMAX);
    return p->n_a >= (size_t)8 * s->n_cu && p->n_sg >= 4 * kg0 && (size_t)4 * k * S <= p->cap;
}

static int mfma_pass_run(mse_searcher* s, const uint16_t* q_dev, int nq_pass, int k, uint64_t id_offset,
                         int64_t* out_scores, uint32_t* out_ids, size_t out_stride, const mse_filter* f, const SparsePlan* sp, bool* overflow);

static int mfma_pass(mse_searcher* s, const uint16_t* q_dev, int nq_pass, int k, uint64_t id_offset,
                     int64_t* out_scores, uint32_t* out_ids, size_t out_stride, const mse_filter* f = nullptr) {
    SparsePlan plan;
    if (sparse_plan(s, nq_pass, k, f, &plan)) {
        bool overflow = false;
        s->last_sparse_passes++;
        if (mfma_pass_run(s, q_dev, nq_pass, k, id_offset, out_scores, out_ids, out_stride, f, &plan, &overflow)) return -1;
        if (!overflow) return 0;
        s->last_sparse_fallbacks++;
    }
    return mfma_pass_run(s, q_dev, nq_pass, k, id_offset, out_scores, out_ids, out_stride, f, nullptr, nullptr);
}

static int mfma_pass_run(mse_searcher* s, const uint16_t* q_dev, int nq_pass, int k, uint64_t id_offset,
                         int64_t* out_scores, uint32_t* out_ids, size_t out_stride, const mse_filter* f, const SparsePlan* sp, bool* overflow) {
    const mse_base* b = s->base;
    hipStream_t st = s->stream;
    const int d = (int)b->d;
    // one pass over the rows serves up to 320 queries (padded to 128 / 192 / 256 / 320); more queries (small base only) = full passes
    // and a last one, their columns side by side in the array of group maxima
    const int tile = mfma_query_tile(d);
    const int n_full = nq_pass / tile, rem = nq_pass - n_full * tile;
    const int nq_pad = n_full * tile + (rem ? mfma_pad(rem, d) : 0);
    if (ensure_base_norm(b, st)) return -1;
    if (reinterpret_cast<uintptr_t>(q_dev) & 15) {   // the kernels read query rows in 16-byte pieces: a misaligned array is copied once
        if (s->q_stage.ensure((size_t)nq_pass * d * 2)) return -1;
        MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, q_dev, (size_t)nq_pass * d * 2, hipMemcpyDeviceToDevice, st));
        q_dev = s->q_stage.as<uint16_t>();
    }
    const int gr = tile == 320 && (!rem || nq_pad - n_full * tile == 320) ? mfma_group_rows(320) : GROUP_ROWS;
    const size_t n_groups = (b->n + gr - 1) / gr;
    if (!sp && s->gmax.ensure(n_groups * (size_t)nq_pad * 4)) return -1;
    // the full passes go out as ONE launch (a small base has few row tiles: its passes fill the chip side by side), then the remainder
    const size_t one_tile_packed = (size_t)(d / 64) * tile * 128;
    if (s->qpacked.ensure(std::max(mfma_packed_bytes(d), (size_t)std::max(n_full, 1) * one_tile_packed))) return -1;
    const uint32_t* mask = f ? f->words : nullptr;
    const size_t mask_words = f ? f->n_words : 0;
    if (s->eps.ensure((size_t)nq_pass * 8) || s->margin.ensure((size_t)nq_pass * 8)) return -1;   // second halves: the widening's compact set
    // the sparse form's lists: thresholds, counts, group ids, maxima (SparsePlan above)
    struct ListSrc { const uint32_t* ids; const float* keys; const uint32_t* counts; const float* tau; };
    ListSrc lists{};
    const uint32_t cap = sp ? sp->cap : 0;
    if (sp) {
        if (s->sp_dense.ensure(sp->n_a * 4 * (size_t)320 * 4) || s->sp_lists.ensure((size_t)320 * 8 + (size_t)320 * cap * 8) ||
            s->sp_pin.ensure((size_t)320 * 4, 4096)) return -1;
        float* tau = s->sp_lists.as<float>();
        uint32_t* counts = reinterpret_cast<uint32_t*>(tau + 320);
        uint32_t* ids = counts + 320;
        float* keys = reinterpret_cast<float*>(ids + (size_t)320 * cap);
        lists = ListSrc{ids, keys, counts, tau};
        ScanSparse a;
        a.n_tiles = sp->n_a; a.mul = sp->stride; a.shift = 63; a.add = 0;
        if (launch_scan_mfma_tiles(b->dev, b->n, d, q_dev, nq_pass, true, s->qpacked.p, a, s->sp_dense.as<float>(), s->n_cu, st,
                                   s->timing ? s->ev0 : nullptr, nullptr)) return -1;
        if (launch_query_eps(q_dev, nq_pass, d, b->norm_bits_dev, 2.8e-4f, s->eps.as<float>(), st)) return -1;
        if (s->gkeys.ensure((size_t)nq_pass * k * 4)) return -1;
        uint32_t* ssel = nullptr;
        LevelRef ls0{KEY_F32, s->sp_dense.p, 1, (size_t)320, sp->n_sg, true, 320};
        if (descend(s, ls0, nq_pass, k, &ssel, s->gkeys.p)) return -1;
        if (launch_sparse_tau(s->gkeys.as<float>(), (size_t)k, k, s->eps.as<float>(), nq_pass, 320, tau, counts, st)) return -1;
        if (launch_sparse_append_sample(s->sp_dense.as<float>(), 320, sp->n_sg, nq_pass, sp->stride, tau, counts, ids, keys, cap, st)) return -1;
        ScanSparse bb;
        bb.n_tiles = sp->n_b; bb.mul = 1; bb.shift = sp->shift; bb.add = 1;   // the j-th tile that is no multiple of S: j + j / (S - 1) + 1
        bb.tau = tau; bb.counts = counts; bb.ids = ids; bb.keys = keys; bb.cap = cap;
        if (launch_scan_mfma_tiles(b->dev, b->n, d, q_dev, nq_pass, false, s->qpacked.p, bb, nullptr, s->n_cu, st, nullptr,
                                   s->timing ? s->ev1 : nullptr)) return -1;
        // the counts reach the host with the first round's margins (its synchronisation)
        MSE_HIP_TRY(hipMemcpyAsync(s->sp_pin.p, counts, (size_t)320 * 4, hipMemcpyDeviceToHost, st));
    }
    if (!sp && n_full &&
        launch_scan_mfma(b->dev, b->n, d, q_dev, tile, s->qpacked.p, s->gmax.as<float>(), s->n_cu, st,
                         s->timing ? s->ev0 : nullptr, s->timing && !rem ? s->ev1 : nullptr, nq_pad, n_full, mask, mask_words, n_full * tile, gr)) return -1;
    if (!sp && rem &&
        launch_scan_mfma(b->dev, b->n, d, q_dev + (size_t)n_full * tile * d, nq_pad - n_full * tile, s->qpacked.p,
                         s->gmax.as<float>() + n_full * tile, s->n_cu, st, s->timing && !n_full ? s->ev0 : nullptr,
                         s->timing ? s->ev1 : nullptr, nq_pad, 1, mask, mask_words, rem, gr)) return -1;
    bool timing_pending = s->timing;
    // |mfma score - exact-order score| <= 2 * gamma_1151 * sum|x_i q_i| <= 1.4e-4 * |x||q|; doubled again
    // because the matrix core's internal rounding is not documented.  (The sparse form needed it for its thresholds already.)
    if (!sp && launch_query_eps(q_dev, nq_pass, d, b->norm_bits_dev, 2.8e-4f, s->eps.as<float>(), st))
        return -1;

    // the margins come back into pinned memory: a true asynchronous copy, then the one synchronisation that ends the round
    if (s->margin_pin.ensure((size_t)nq_pass * 4, 4096)) return -1;
    float* const margin_h = s->margin_pin.as<float>();
    const int kg0 = (int)std::min<size_t>(std::max(k + 8, 16), TOPK_KMAX);
    s->last_widened = 0;
    // One round of: tournament over the group maxima -> the kg best groups' rows re-scored exactly -> exact top-k -> certificate.
    // gm: group maxima [n_groups][gm_pad] of the nq queries in `qs` ([nq][d] f16); results go to dst_* with stride dst_stride;
    // margins (> 0 = certified) come back in margin_h[0..nq).
    // ls (the sparse form): the kg best groups come from the queries' lists instead of a tournament over gm
    auto round = [&](const float* gm, int gm_pad, const ListSrc* ls, const uint16_t* qs, int nq, int kg_eff, const float* eps_dev, float* margin_dev,
                     int64_t* dst_s, uint32_t* dst_i, size_t dst_stride, uint64_t id_off) -> int {
        if (s->gkeys.ensure((size_t)nq * kg_eff * 4)) return -1;
        uint32_t* gsel = nullptr;
        if (ls) {
            if (s->sel_a.ensure((size_t)nq * kg_eff * 4)) return -1;
            gsel = s->sel_a.as<uint32_t>();
            SelectArgs a{};
            a.kind = KEY_F32; a.list_ids = ls->ids; a.list_keys = ls->keys; a.list_stride = cap; a.n_list = cap; a.list_count = ls->counts;
            a.k = kg_eff; a.out_ids = gsel; a.out_keys = s->gkeys.p; a.out_stride = kg_eff; a.nq = nq;
            if (launch_select(a, st)) return -1;
        } else {
            LevelRef l0{KEY_F32, gm, 1, (size_t)gm_pad, n_groups, true, gm_pad};
            if (descend(s, l0, nq, kg_eff, &gsel, s->gkeys.p)) return -1;
        }
        const size_t n_cand = (size_t)kg_eff * gr;
        if (s->cand_ids.ensure((size_t)nq * n_cand * 4) || s->cand_scores.ensure((size_t)nq * n_cand * 8)) return -1;
        if (f ? launch_expand_groups_masked(gsel, kg_eff, kg_eff, gr, b->n, f->words, f->n_words, s->cand_ids.as<uint32_t>(), n_cand,
                                            nq, st)
              : launch_expand_groups(gsel, kg_eff, kg_eff, gr, b->n, s->cand_ids.as<uint32_t>(), n_cand, nq, st)) return -1;
        if (launch_score_rows(b->dev, b->n, d, qs, false, s->cand_ids.as<uint32_t>(), (size_t)nq * n_cand, n_cand,
                              s->cand_scores.as<int64_t>(), nullptr, st)) return -1;
        // final exact selection among the re-scored candidates
        if (s->sel_keys.ensure((size_t)nq * k * 8) || s->misc.ensure((size_t)nq * k * 4)) return -1;
        SelectArgs a{};
        a.kind = KEY_I64; a.list_ids = s->cand_ids.as<uint32_t>(); a.list_keys = s->cand_scores.p;
        a.list_stride = n_cand; a.n_list = n_cand; a.k = k; a.out_ids = s->misc.as<uint32_t>();
        a.out_keys = s->sel_keys.p; a.out_stride = k; a.nq = nq;
        if (launch_select(a, st)) return -1;
        if (launch_finalize(s->misc.as<uint32_t>(), s->sel_keys.as<int64_t>(), k, k, nq, id_off, dst_s, dst_i, dst_stride,
                            s->gkeys.as<float>(), kg_eff, kg_eff, n_groups, eps_dev, margin_dev, st, ls ? ls->tau : nullptr)) return -1;
        MSE_HIP_TRY(hipMemcpyAsync(margin_h, margin_dev, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        MSE_HIP_TRY(hipStreamSynchronize(st));
        s->last_max_groups = std::max<uint32_t>(s->last_max_groups, (uint32_t)kg_eff);
        return 0;
    };
    if (round(sp ? nullptr : s->gmax.as<float>(), nq_pad, sp ? &lists : nullptr, q_dev, nq_pass, kg0, s->eps.as<float>(), s->margin.as<float>(),
              out_scores, out_ids, out_stride, id_offset)) return -1;
    if (timing_pending) {
        // (the sparse form: from the start of launch A to the end of launch B, the small kernels between them included)
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) { s->scan_ms_total += ms; s->scan_launches++; }
        timing_pending = false;
    }
    const uint32_t* const counts_h = sp ? s->sp_pin.as<uint32_t>() : nullptr;
    if (sp) {
        uint32_t longest = 0;
        for (int i = 0; i < nq_pass; i++) longest = std::max(longest, counts_h[i]);
        s->last_sparse_max_list = std::max(s->last_sparse_max_list, longest);
        if (longest > cap) { *overflow = true; return 0; }   // a list lost survivors: nothing of this attempt stands
    }
    std::vector<uint32_t> bad;
    for (int i = 0; i < nq_pass; i++)
        if (!(margin_h[i] > 0.0f)) bad.push_back((uint32_t)i);
    if (bad.empty() || (size_t)kg0 >= n_groups) return 0;
    s->last_widened = (uint32_t)bad.size();
    // The queries whose certificate failed (near-duplicate rows around their k-th score, ties) are carried on as a COMPACT set: their
    // columns of the group maxima, their query rows.  Widening then costs what those few queries cost -- not a 4x, 16x, 64x larger
    // re-score for all 256 (a clustered 1e8-row set: 84 ms per pass of 256 queries instead of 58, before this).
    const int nb = (int)bad.size(), nbp = (nb + 31) / 32 * 32;
    if (s->widx.ensure((size_t)nb * 5) || s->wq.ensure((size_t)(nb + 8) * d * 2) || (!sp && s->wg.ensure(n_groups * (size_t)nbp * 4)) ||
        s->wout.ensure((size_t)std::max(nb, 8) * k * 12)) return -1;
    uint32_t* idx_dev = s->widx.as<uint32_t>();
    uint8_t* take_dev = reinterpret_cast<uint8_t*>(idx_dev + nb);
    MSE_HIP_TRY(hipMemcpyAsync(idx_dev, bad.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
    if (launch_gather_rows16(q_dev, (size_t)d * 2, idx_dev, nb, s->wq.p, st)) return -1;
    ListSrc wlists{};
    size_t longest_bad = 0;   // the sparse form: the longest list of the compact set -- more groups than that widen nothing
    if (sp) {
        if (s->sp_wlists.ensure((size_t)nb * 8 + (size_t)nb * cap * 8)) return -1;
        float* tau = s->sp_wlists.as<float>();
        uint32_t* counts = reinterpret_cast<uint32_t*>(tau + nb);
        uint32_t* ids = counts + nb;
        float* keys = reinterpret_cast<float*>(ids + (size_t)nb * cap);
        wlists = ListSrc{ids, keys, counts, tau};
        if (launch_sparse_gather_lists(lists.ids, lists.keys, lists.counts, lists.tau, cap, idx_dev, nb, ids, keys, counts, tau, st)) return -1;
        for (uint32_t i : bad) longest_bad = std::max<size_t>(longest_bad, counts_h[i]);
    } else if (launch_gather_columns(s->gmax.as<float>(), nq_pad, n_groups, idx_dev, nb, s->wg.as<float>(), nbp, st)) return -1;
    float* eps2 = s->eps.as<float>() + nq_pass;
    float* margin2 = s->margin.as<float>() + nq_pass;
    if (launch_query_eps(s->wq.as<uint16_t>(), nb, d, b->norm_bits_dev, 2.8e-4f, eps2, st)) return -1;
    int64_t* w_s = s->wout.as<int64_t>();
    uint32_t* w_i = reinterpret_cast<uint32_t*>(s->wout.as<char>() + (size_t)nb * k * 8);
    std::vector<uint8_t> open_q(nb, 1);   // still uncertified
    int kg = kg0 * 4;
    for (;;) {
        const int kg_eff = (int)std::min<size_t>(kg, TOPK_KMAX);
        if (round(sp ? nullptr : s->wg.as<float>(), nbp, sp ? &wlists : nullptr, s->wq.as<uint16_t>(), nb, kg_eff, eps2, margin2, w_s, w_i, (size_t)k,
                  id_offset)) return -1;
        // rows of the queries certified in this round (or examined completely) go to their places
        std::vector<uint8_t> take(nb, 0);
        int still = 0;
        for (int j = 0; j < nb; j++) {
            if (!open_q[j]) continue;
            if (margin_h[j] > 0.0f || (size_t)kg_eff >= n_groups) { take[j] = 1; open_q[j] = 0; } else still++;
        }
        MSE_HIP_TRY(hipMemcpyAsync(take_dev, take.data(), (size_t)nb, hipMemcpyHostToDevice, st));
        if (launch_scatter_topk(idx_dev, take_dev, nb, k, w_s, w_i, out_scores, out_ids, out_stride, st)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(st));   // `take` is a stack-owned source
        if (still == 0) return 0;
        // (a list used up leaves the threshold as the bound, which certifies by construction: the second test is a safety net that
        // sends what is still open -- a k-th score saturated to INT64_MIN, which proves nothing -- to the exact scan)
        if (kg_eff >= TOPK_KMAX || (sp && (size_t)kg_eff >= longest_bad)) break;
        kg = kg_eff * 4;
    }
    // cannot widen further: the exact scan for what is left, 8 queries at a time
    std::vector<uint32_t> rest;
    for (int j = 0; j < nb; j++)
        if (open_q[j]) rest.push_back((uint32_t)j);
    for (size_t r0 = 0; r0 < rest.size(); r0 += 8) {
        const int nqp = (int)std::min<size_t>(8, rest.size() - r0);
        if (s->q_stage.ensure((size_t)8 * d * 2)) return -1;
        MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, (size_t)8 * d * 2, st));
        for (int j = 0; j < nqp; j++)
            MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.as<char>() + (size_t)j * d * 2, s->wq.as<char>() + (size_t)rest[r0 + j] * d * 2, (size_t)d * 2,
                                       hipMemcpyDeviceToDevice, st));
        if (exact_pass(s, nqp, k, id_offset, w_s, w_i, (size_t)k, f)) return -1;
        std::vector<uint32_t> dst(nqp);
        for (int j = 0; j < nqp; j++) dst[j] = bad[rest[r0 + j]];
        MSE_HIP_TRY(hipMemcpyAsync(idx_dev, dst.data(), (size_t)nqp * 4, hipMemcpyHostToDevice, st));
        if (launch_scatter_topk(idx_dev, nullptr, nqp, k, w_s, w_i, out_scores, out_ids, out_stride, st)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

// The sparse path: scoring the filter's id list directly (exact_pass: the list is read once per 8 queries) beats the masked scan (every
// row streamed once per pass) when count x ceil(nq / 8) x 3 <= n_rows x ceil(nq / pass width) x 2.  Measured on one MI355X, 1e8 x 1152
// (scripts/filtered_scan_probe.py, profiles/filtered_scan_probe.json): the list pass costs 0.56 ns per listed row per 8 queries, the
// masked scan 0.40 ns per row per pass of <= 128 queries and 0.74 ns at 320 -- e.g. 1.6e6 allowed rows x 320 queries: list 35 ms,
// scan 74 ms; 6.3e6 x 64: 28 against 40 ms; 1.25e7 x 64: 57 against 40 ms.  The factor 3 / 2 sits between those costs.
bool filter_sparse(const mse_base* b, const mse_filter* f, size_t nq) {
    const size_t tile = (size_t)mfma_query_tile((int)b->d);
    return f->count * ((nq + 7) / 8) * 3 <= b->n * ((nq + tile - 1) / tile) * 2;
}

int check_filter(const mse_base* b, const mse_filter* f) {
    if (!f) return fail("null filter");
    if (f->n_rows > b->n) return fail("filter is longer than the base (" + std::to_string(f->n_rows) + " > " + std::to_string(b->n) + " rows)");
    if (f->device != b->device) return fail("filter was made on another device than the base's");   // no silent copy
    return 0;
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
    for (hipEvent_t e : s->ev_pool) (void)hipEventDestroy(e);
    if (s->ev_wait) (void)hipEventDestroy(s->ev_wait);
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

// every one of the [nq][k] output slots empty (INT64_MIN / MSE_ID_NONE)
static int fill_empty(mse_searcher* s, size_t nq, size_t k, int64_t* out_scores, uint32_t* out_ids) {
    std::vector<int64_t> hs(nq * k, INT64_MIN);
    std::vector<uint32_t> hi(nq * k, MSE_ID_NONE);
    MSE_HIP_TRY(hipMemcpyAsync(out_scores, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(out_ids, hi.data(), hi.size() * 4, hipMemcpyHostToDevice, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

int mse_bruteforce_topk_f16_dev(mse_searcher* s, const void* queries_dev, size_t nq, size_t k, int mode,
                                uint64_t id_offset, void* scores_dev, void* ids_dev) {
    if (!s) return fail("null searcher");
    if (nq == 0 || k == 0) return 0;
    if (k > (size_t)TOPK_KMAX - 64) return fail("k too large (max 1984)");
    const mse_base* b = s->base;
    const int d = (int)b->d;
    int64_t* out_scores = reinterpret_cast<int64_t*>(scores_dev);
    uint32_t* out_ids = reinterpret_cast<uint32_t*>(ids_dev);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(queries_dev);
    if (mode == MSE_MODE_AUTO) mode = nq <= 8 ? MSE_MODE_EXACT : MSE_MODE_MFMA;
    s->last_widened = 0;
    s->last_max_groups = 0;
    s->last_sparse_passes = s->last_sparse_fallbacks = s->last_sparse_max_list = 0;
    if (b->n == 0) return fill_empty(s, nq, k, out_scores, out_ids);   // nothing to score
    if (mode == MSE_MODE_EXACT) {
        for (size_t q0 = 0; q0 < nq; q0 += 8) {
            const int nqp = (int)std::min<size_t>(8, nq - q0);
            if (s->q_stage.ensure((size_t)8 * d * 2)) return -1;
            MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, (size_t)8 * d * 2, s->stream));
            MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, q + q0 * d, (size_t)nqp * d * 2, hipMemcpyDeviceToDevice, s->stream));
            if (exact_pass(s, nqp, (int)k, id_offset, out_scores + q0 * k, out_ids + q0 * k, k)) return -1;
        }
        return 0;
    }
    if (mode == MSE_MODE_MFMA) {
        const size_t tile = mfma_call_tile(b, k);
        for (size_t q0 = 0; q0 < nq; q0 += tile) {
            const int nqp = (int)std::min<size_t>(tile, nq - q0);
            if (mfma_pass(s, q + q0 * d, nqp, (int)k, id_offset, out_scores + q0 * k, out_ids + q0 * k, k)) return -1;
        }
        return 0;
    }
    return fail("unknown mode");
}

// test hook: the raw output of the matrix-core scan, so that its deviation from the exact-order scores can be MEASURED
// (tests/test_gpu_bruteforce.py) instead of assumed: out[g][q] = max over rows 32g .. 32g+31 of the MFMA score of query q
int mse_debug_mfma_group_max(mse_searcher* s, const uint16_t* queries, size_t nq, float* out) {
    if (!s || !s->base) return fail("null searcher");
    const mse_base* b = s->base;
    if (nq == 0 || nq > (size_t)mfma_query_tile((int)b->d) || b->n == 0) return fail("mfma_group_max: 1..320 queries (256 when d / 64 is odd), non-empty base");
    const int d = (int)b->d;
    const int nq_pad = mfma_pad((int)nq, d);
    const size_t n_groups = (b->n + GROUP_ROWS - 1) / GROUP_ROWS;
    if (s->q_stage.ensure((size_t)nq_pad * d * 2) || s->gmax.ensure(n_groups * (size_t)nq_pad * 4) ||
        s->qpacked.ensure(mfma_packed_bytes(d))) return -1;
    MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, (size_t)nq_pad * d * 2, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, queries, nq * d * 2, hipMemcpyHostToDevice, s->stream));
    if (launch_scan_mfma(b->dev, b->n, d, s->q_stage.as<uint16_t>(), nq_pad, s->qpacked.p, s->gmax.as<float>(), s->n_cu, s->stream))
        return -1;
    MSE_HIP_TRY(hipMemcpy2DAsync(out, nq * 4, s->gmax.p, (size_t)nq_pad * 4, nq * 4, n_groups, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

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

// the base's coalescer, made on first use (null if it cannot be made: callers then answer directly)
static mse_dispatcher* base_dispatcher(const mse_base* b) {
    std::lock_guard<std::mutex> g(b->disp_mu);
    if (!b->disp && !b->disp_failed) {
        b->disp = mse_dispatcher_new(b, 0, 0);
        if (!b->disp) b->disp_failed = true;
    }
    return b->disp;
}

int mse_bruteforce_topk_f16(mse_searcher* s, const uint16_t* queries, size_t nq, size_t k, int mode, int64_t* scores,
                            uint32_t* ids) {
    if (!s) return fail("null searcher");
    if (nq == 0 || k == 0) return 0;
    if (mode == MSE_MODE_AUTO && s->base && nq <= (size_t)mfma_query_tile((int)s->base->d)) {
        // The reference's call shape is a thread per core, each with its own Scratch and ONE query per request
        // (src/query_disk_index.rs:711-736): such callers meet in the base's coalescer and share a pass over the rows.
        // Answers are those of every other mode; a lone caller fires its pass at once (dispatch.h).  Only requests that fit one pass
        // go there: a larger batch fills passes on its own and stays on the caller's searcher (its stream, its timing, its
        // last_stats).  If the coalescer cannot be made (no memory for its worker's scratch) the call is answered directly as well.
        mse_dispatcher* disp = base_dispatcher(s->base);
        if (disp) return mse_dispatcher_topk_f16(disp, queries, nq, k, scores, ids);
    }
    const size_t d = s->base->d;
    DevBuf qd;
    if (qd.ensure(nq * d * 2)) return -1;
    if (s->out_scores.ensure(nq * k * 8) || s->out_ids.ensure(nq * k * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(qd.p, queries, nq * d * 2, hipMemcpyHostToDevice, s->stream));
    if (mse_bruteforce_topk_f16_dev(s, qd.p, nq, k, mode, 0, s->out_scores.p, s->out_ids.p)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(scores, s->out_scores.p, nq * k * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(ids, s->out_ids.p, nq * k * 4, hipMemcpyDeviceToHost, s->stream));
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

int mse_bruteforce_scores_f16(mse_searcher* s, const uint16_t* query, int64_t* scores) {
    if (!s) return fail("null searcher");
    const mse_base* b = s->base;
    if (b->n == 0) return 0;
    const size_t d = b->d;
    if (s->q_stage.ensure(8 * d * 2) || s->scores.ensure(b->n * 8)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, 8 * d * 2, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, query, d * 2, hipMemcpyHostToDevice, s->stream));
    if (launch_scan_exact(b->dev, b->n, (int)d, s->q_stage.p, 1, false, s->scores.as<int64_t>(), b->n, nullptr, s->n_cu,
                          s->stream)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(scores, s->scores.p, b->n * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

int mse_score_rows_f16(mse_searcher* s, const uint32_t* ids, size_t n_ids, const uint16_t* query, int64_t* out) {
    if (!s) return fail("null searcher");
    if (n_ids == 0) return 0;
    const mse_base* b = s->base;
    const size_t d = b->d;
    if (s->q_stage.ensure(8 * d * 2) || s->cand_ids.ensure(n_ids * 4) || s->cand_scores.ensure(n_ids * 8)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, query, d * 2, hipMemcpyHostToDevice, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(s->cand_ids.p, ids, n_ids * 4, hipMemcpyHostToDevice, s->stream));
    if (launch_score_rows(b->dev, b->n, (int)d, s->q_stage.p, false, s->cand_ids.as<uint32_t>(), n_ids, n_ids,
                          s->cand_scores.as<int64_t>(), nullptr, s->stream)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(out, s->cand_scores.p, n_ids * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

// ---- row filters (filter.hip) and the filtered brute-force search -----------------------------------------------------------

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
// the thread's current device for the length of a call that must build on another one
struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

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



int mse_bruteforce_topk_filtered_f16_dev(mse_searcher* s, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode,
                                         uint64_t id_offset, void* scores_dev, void* ids_dev) {
    if (!s) return fail("null searcher");
    if (check_filter(s->base, f)) return -1;
    if (nq == 0 || k == 0) return 0;
    if (k > (size_t)TOPK_KMAX - 64) return fail("k too large (max 1984)");
    if (mode != MSE_MODE_AUTO && mode != MSE_MODE_EXACT && mode != MSE_MODE_MFMA) return fail("unknown mode");
    const mse_base* b = s->base;
    const int d = (int)b->d;
    int64_t* out_scores = reinterpret_cast<int64_t*>(scores_dev);
    uint32_t* out_ids = reinterpret_cast<uint32_t*>(ids_dev);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(queries_dev);
    s->last_widened = 0;
    s->last_max_groups = 0;
    s->last_sparse_passes = s->last_sparse_fallbacks = s->last_sparse_max_list = 0;
    if (f->count == 0) return fill_empty(s, nq, k, out_scores, out_ids);   // nothing allowed
    // MODE_EXACT: the filtered exact pass.  MODE_MFMA: the masked matrix-core scan.  MODE_AUTO: the exact pass on the sparse side of the
    // crossover; otherwise the unfiltered rule (the coalescer's, dispatch.hip): the masked scan for more than 8 queries, and for any
    // count once the rows have outgrown the caches.  Answers are identical on every path.
    if (mode == MSE_MODE_AUTO)
        mode = filter_sparse(b, f, nq) ? MSE_MODE_EXACT : (nq > 8 || b->n >= ((size_t)1 << 22)) ? MSE_MODE_MFMA : MSE_MODE_EXACT;
    if (mode == MSE_MODE_EXACT) {
        for (size_t q0 = 0; q0 < nq; q0 += 8) {
            const int nqp = (int)std::min<size_t>(8, nq - q0);
            if (s->q_stage.ensure((size_t)8 * d * 2)) return -1;
            MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, (size_t)8 * d * 2, s->stream));
            MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, q + q0 * d, (size_t)nqp * d * 2, hipMemcpyDeviceToDevice, s->stream));
            if (exact_pass(s, nqp, (int)k, id_offset, out_scores + q0 * k, out_ids + q0 * k, k, f)) return -1;
        }
        return 0;
    }
    const size_t tile = mfma_call_tile(b, k);
    for (size_t q0 = 0; q0 < nq; q0 += tile) {
        const int nqp = (int)std::min<size_t>(tile, nq - q0);
        if (mfma_pass(s, q + q0 * d, nqp, (int)k, id_offset, out_scores + q0 * k, out_ids + q0 * k, k, f)) return -1;
    }
    return 0;
}

int mse_bruteforce_topk_filtered_f16(mse_searcher* s, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k, int mode,
                                     int64_t* scores, uint32_t* ids) {
    if (!s) return fail("null searcher");
    if (check_filter(s->base, f)) return -1;
    if (nq == 0 || k == 0) return 0;
    if (k > (size_t)TOPK_KMAX - 64) return fail("k too large (max 1984)");
    if (mode == MSE_MODE_AUTO && nq <= (size_t)mfma_query_tile((int)s->base->d)) {
        // as mse_bruteforce_topk_f16: the base's coalescer, where the request shares a pass with the requests of the same filter
        mse_dispatcher* disp = base_dispatcher(s->base);
        if (disp) return mse_dispatcher_topk_filtered_f16(disp, f, queries, nq, k, scores, ids);
    }
    const size_t d = s->base->d;
    DevBuf qd;
    if (qd.ensure(nq * d * 2)) return -1;
    if (s->out_scores.ensure(nq * k * 8) || s->out_ids.ensure(nq * k * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(qd.p, queries, nq * d * 2, hipMemcpyHostToDevice, s->stream));
    if (mse_bruteforce_topk_filtered_f16_dev(s, f, qd.p, nq, k, mode, 0, s->out_scores.p, s->out_ids.p)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(scores, s->out_scores.p, nq * k * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(ids, s->out_ids.p, nq * k * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

}  // extern "C"
