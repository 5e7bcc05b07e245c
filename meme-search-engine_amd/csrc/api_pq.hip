// C ABI, part 2: evaluator ranks, flat fp16 index (FAISS SQfp16-IP semantics), product quantiser.
#include "../../include/mse.h"
#include "runtime.h"
#include "dispatch.h"
#include <algorithm>
#include <atomic>
#include <memory>
#include <cfloat>
#include <cstring>
#include <new>
#include <vector>

using namespace mse;

// Flat index.  Concurrency is the reference's: searches share, `add` excludes (the RwLock of src/main.rs:1016 write / :1046
// read).  Searches of all threads meet in the index's coalescer (dispatch.h) and are executed by its ONE worker thread, which
// is the only user of `scratch` while readers hold the lock; `add` runs on the caller's thread with every reader out.
struct mse_index {
    int d = 0;
    int device = 0;
    size_t n = 0, cap = 0;
    uint16_t* codes = nullptr;   // [cap][d] fp16, device
    mse_base view;               // non-owning view of codes[0..n) for the matrix-core scan; its norm bound grows with every add
    mse_searcher* scratch = nullptr;
    mse::SharedExclusive rw;
    std::unique_ptr<mse::Coalescer> co;
    mse::PinBuf pin;             // pinned staging of the worker: queries up, [distances | labels] down
    mse::DevBuf q32, out;
    std::atomic<uint64_t> retried_alone{0};
};

extern "C" {

// ---- evaluator ranks (src/query_disk_index.rs:271-273,309-316) ---------------------------------
int mse_bruteforce_ranks_f16(mse_searcher* s, const uint16_t* query, const uint32_t* ids, size_t n_ids,
                             uint32_t* ranks) {
    if (!s || !s->base) return fail("null searcher");
    const mse_base* b = s->base;
    if (n_ids == 0) return 0;
    const size_t d = b->d;
    hipStream_t st = s->stream;
    if (s->q_stage.ensure(8 * d * 2) || s->scores.ensure(std::max<size_t>(b->n, 1) * 8)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, 8 * d * 2, st));
    MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, query, d * 2, hipMemcpyHostToDevice, st));
    if (launch_scan_exact(b->dev, b->n, (int)d, s->q_stage.p, 1, false, s->scores.as<int64_t>(), b->n, nullptr, s->n_cu,
                          st)) return -1;
    const size_t chunk = (size_t)rank_max_targets();
    if (s->cand_ids.ensure(chunk * 4) || s->cand_scores.ensure(chunk * 8)) return -1;
    std::vector<unsigned long long> counts(chunk);
    for (size_t o = 0; o < n_ids; o += chunk) {
        const size_t m = std::min(chunk, n_ids - o);
        for (size_t i = 0; i < m; i++)
            if (ids[o + i] >= b->n) return fail("rank: id out of range");
        MSE_HIP_TRY(hipMemcpyAsync(s->cand_ids.p, ids + o, m * 4, hipMemcpyHostToDevice, st));
        MSE_HIP_TRY(hipMemsetAsync(s->cand_scores.p, 0, m * 8, st));
        if (launch_rank(s->scores.as<int64_t>(), b->n, s->cand_ids.as<uint32_t>(), (int)m,
                        s->cand_scores.as<unsigned long long>(), s->n_cu, st)) return -1;
        MSE_HIP_TRY(hipMemcpyAsync(counts.data(), s->cand_scores.p, m * 8, hipMemcpyDeviceToHost, st));
        MSE_HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < m; i++) ranks[o + i] = (uint32_t)counts[i];
    }
    return 0;
}

// ---- flat index -----------------------------------------------------------------------------------
namespace {

// <= 8 f32 queries against every row in the stated FAISS order (scan_exact.hip, QF32), tournament, ids + f32 keys into
// out_ids / out_keys ([nq][out_stride], ID_NONE-padded)
// With a filter (non-empty, no longer than the index): its allowed rows only, through its ascending id list (bruteforce.hip exact_pass).
// With a grouping: the dense path of the grouped search (bruteforce.hip grouped_dense_pass, on f32 keys) -- the best row of every group
// by ONE 8-byte atomic max of (order-preserving key << 32) | ~row per row, which decides distance and label at once; every other
// grouped row drops out of the ranking; the selection's k results are collapsed (a demoted row that fills a short list comes after its
// own representative) and go to row dst_rows[j] (device; null: j) of the outputs.
int index_pass_exact(mse_index* idx, const float* q32_dev, int nqp, int k, uint32_t* out_ids, float* out_keys, size_t out_stride,
                     const mse_filter* f = nullptr, const mse_groups* g = nullptr, const uint32_t* dst_rows = nullptr) {
    mse_searcher* s = idx->scratch;
    hipStream_t st = s->stream;
    const size_t d = idx->d, n = f ? f->count : idx->n;
    if (s->q_stage.ensure(8 * d * 4) || s->scores.ensure((size_t)nqp * n * 4)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, 8 * d * 4, st));
    MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, q32_dev, (size_t)nqp * d * 4, hipMemcpyDeviceToDevice, st));
    if (launch_scan_exact(idx->codes, n, (int)d, s->q_stage.p, nqp, true, nullptr, n, s->scores.as<float>(), s->n_cu, st,
                          f ? f->ids : nullptr)) return -1;
    if (g && g->n_rows) {
        if (s->grp_best.ensure((size_t)nqp * g->n_rows * 8)) return -1;
        if (launch_dense_group_best(true, s->scores.p, n, n, f ? f->ids : nullptr, g->group_of, g->n_rows, nqp, s->grp_best.as<unsigned long long>(),
                                    nullptr, nullptr, st)) return -1;
    }
    if (s->sel_keys.ensure((size_t)nqp * k * 4)) return -1;
    uint32_t* sel = nullptr;
    LevelRef l0{KEY_F32, s->scores.p, n, 1, n, false, 0};
    if (descend(s, l0, nqp, k, &sel, s->sel_keys.p)) return -1;
    if (f && launch_map_positions(sel, (size_t)nqp * k, f->ids, st)) return -1;
    if (g) {
        if (s->grp_pos.ensure((size_t)nqp * k * 4) || s->grp_reps.ensure((size_t)nqp * 4)) return -1;
        if (launch_collapse(sel, (size_t)k, (size_t)k, g->group_of, g->n_rows, k, nqp, s->grp_pos.as<uint32_t>(), s->grp_reps.as<uint32_t>(), st)) return -1;
        return launch_collapse_gather(s->grp_pos.as<uint32_t>(), k, sel, (size_t)k, s->sel_keys.p, (size_t)k, 4, nqp, 0, dst_rows, nullptr, out_keys,
                                      out_ids, out_stride, st);
    }
    MSE_HIP_TRY(hipMemcpy2DAsync(out_ids, out_stride * 4, sel, (size_t)k * 4, (size_t)k * 4, nqp, hipMemcpyDeviceToDevice, st));
    MSE_HIP_TRY(hipMemcpy2DAsync(out_keys, out_stride * 4, s->sel_keys.p, (size_t)k * 4, (size_t)k * 4, nqp, hipMemcpyDeviceToDevice, st));
    return 0;
}

// Up to 256 f32 queries in ONE pass over the rows.  The matrix cores score f16 roundings of the queries and only nominate:
// group maxima -> tournament -> the rows of the best groups re-scored with the f32 query in the stated order -> top k ->
// certificate.  The bound on what the nomination can have missed is the f16 scan's (bruteforce.hip mfma_pass) plus the query
// rounding, |x . (q - f16(q))| <= |x| |q - f16(q)| (measured per query, not assumed).  A query whose certificate fails widens
// its candidate set and finally repeats through the exact pass: answers equal index_pass_exact's.
// With a filter: the masked scan, excluded rows dropped at candidate expansion, the filtered exact pass as the fallback (bruteforce.hip mfma_pass).
int index_pass_mfma(mse_index* idx, const float* q32_dev, int nqp, int k, uint32_t* out_ids, float* out_keys, size_t out_stride,
                    const mse_filter* f = nullptr) {
    mse_searcher* s = idx->scratch;
    hipStream_t st = s->stream;
    const int d = idx->d;
    const size_t n = idx->n;
    const int nq_pad = mfma_pad(nqp, d);
    if (s->q_stage.ensure((size_t)nq_pad * d * 2)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, (size_t)nq_pad * d * 2, st));
    if (launch_f32_to_f16(q32_dev, (size_t)nqp * d, s->q_stage.as<uint16_t>(), st)) return -1;
    const size_t n_groups = (n + GROUP_ROWS - 1) / GROUP_ROWS;
    if (s->gmax.ensure(n_groups * (size_t)nq_pad * 4) || s->qpacked.ensure(mfma_packed_bytes(d))) return -1;
    if (launch_scan_mfma(idx->codes, n, d, s->q_stage.as<uint16_t>(), nq_pad, s->qpacked.p, s->gmax.as<float>(), s->n_cu, st,
                         s->timing ? s->ev0 : nullptr, s->timing ? s->ev1 : nullptr, 0, 1, f ? f->words : nullptr, f ? f->n_words : 0))
        return -1;
    bool timing_pending = s->timing;
    if (s->eps.ensure((size_t)nqp * 8) || s->margin.ensure((size_t)nqp * 8)) return -1;   // second halves: the widening's compact set
    if (launch_query_eps_f32(q32_dev, s->q_stage.as<uint16_t>(), nqp, d, idx->view.norm_bits_dev, 2.8e-4f, s->eps.as<float>(), st)) return -1;
    std::vector<float> margin_h(nqp);
    const int kg0 = (int)std::min<size_t>(std::max(k + 8, 16), TOPK_KMAX);
    // one round: tournament -> rows of the kg best groups re-scored with the f32 queries -> top k -> certificate margins (host)
    auto round = [&](const float* gm, int gm_pad, const float* q32, int nq, int kg_eff, const float* eps_dev, float* margin_dev, uint32_t* dst_i,
                     float* dst_k, size_t dst_stride) -> int {
        if (s->gkeys.ensure((size_t)nq * kg_eff * 4)) return -1;
        uint32_t* gsel = nullptr;
        LevelRef l0{KEY_F32, gm, 1, (size_t)gm_pad, n_groups, true, gm_pad};
        if (descend(s, l0, nq, kg_eff, &gsel, s->gkeys.p)) return -1;
        const size_t n_cand = (size_t)kg_eff * GROUP_ROWS;
        if (s->cand_ids.ensure((size_t)nq * n_cand * 4) || s->cand_scores.ensure((size_t)nq * n_cand * 4)) return -1;
        if (f ? launch_expand_groups_masked(gsel, kg_eff, kg_eff, GROUP_ROWS, n, f->words, f->n_words, s->cand_ids.as<uint32_t>(), n_cand, nq, st)
              : launch_expand_groups(gsel, kg_eff, kg_eff, GROUP_ROWS, n, s->cand_ids.as<uint32_t>(), n_cand, nq, st)) return -1;
        if (launch_score_rows(idx->codes, n, d, q32, true, s->cand_ids.as<uint32_t>(), (size_t)nq * n_cand, n_cand, nullptr,
                              s->cand_scores.as<float>(), st)) return -1;
        SelectArgs a{};
        a.kind = KEY_F32; a.list_ids = s->cand_ids.as<uint32_t>(); a.list_keys = s->cand_scores.p;
        a.list_stride = n_cand; a.n_list = n_cand; a.k = k; a.out_ids = dst_i; a.out_keys = dst_k; a.out_stride = dst_stride; a.nq = nq;
        if (launch_select(a, st)) return -1;
        if (launch_margin_f32(dst_i, dst_k, dst_stride, k, nq, s->gkeys.as<float>(), kg_eff, kg_eff, n_groups, eps_dev, margin_dev, st)) return -1;
        MSE_HIP_TRY(hipMemcpyAsync(margin_h.data(), margin_dev, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        MSE_HIP_TRY(hipStreamSynchronize(st));
        s->last_max_groups = std::max<uint32_t>(s->last_max_groups, (uint32_t)kg_eff);
        return 0;
    };
    if (round(s->gmax.as<float>(), nq_pad, q32_dev, nqp, kg0, s->eps.as<float>(), s->margin.as<float>(), out_ids, out_keys, out_stride)) return -1;
    if (timing_pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) { s->scan_ms_total += ms; s->scan_launches++; }
        timing_pending = false;
    }
    std::vector<uint32_t> bad;
    for (int i = 0; i < nqp; i++)
        if (!(margin_h[i] > 0.0f)) bad.push_back((uint32_t)i);
    if (bad.empty() || (size_t)kg0 >= n_groups) return 0;
    s->last_widened = std::max<uint32_t>(s->last_widened, (uint32_t)bad.size());
    // only the queries whose certificate failed go on, as a compact set (bruteforce.hip mfma_pass has the same structure)
    const int nb = (int)bad.size(), nbp = (nb + 31) / 32 * 32;
    if (s->widx.ensure((size_t)nb * 5) || s->wq.ensure((size_t)nb * d * 6) || s->wg.ensure(n_groups * (size_t)nbp * 4) ||
        s->wout.ensure((size_t)nb * k * 8)) return -1;
    uint32_t* idx_dev = s->widx.as<uint32_t>();
    uint8_t* take_dev = reinterpret_cast<uint8_t*>(idx_dev + nb);
    float* wq32 = s->wq.as<float>();
    uint16_t* wq16 = reinterpret_cast<uint16_t*>(s->wq.as<char>() + (size_t)nb * d * 4);
    MSE_HIP_TRY(hipMemcpyAsync(idx_dev, bad.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
    if (launch_gather_rows16(q32_dev, (size_t)d * 4, idx_dev, nb, wq32, st)) return -1;
    if (launch_gather_rows16(s->q_stage.p, (size_t)d * 2, idx_dev, nb, wq16, st)) return -1;
    if (launch_gather_columns(s->gmax.as<float>(), nq_pad, n_groups, idx_dev, nb, s->wg.as<float>(), nbp, st)) return -1;
    float* eps2 = s->eps.as<float>() + nqp;
    float* margin2 = s->margin.as<float>() + nqp;
    if (launch_query_eps_f32(wq32, wq16, nb, d, idx->view.norm_bits_dev, 2.8e-4f, eps2, st)) return -1;
    uint32_t* w_i = s->wout.as<uint32_t>();
    float* w_k = reinterpret_cast<float*>(s->wout.as<char>() + (size_t)nb * k * 4);
    std::vector<uint8_t> open_q(nb, 1);
    int kg = kg0 * 4;
    for (;;) {
        const int kg_eff = (int)std::min<size_t>(kg, TOPK_KMAX);
        if (round(s->wg.as<float>(), nbp, wq32, nb, kg_eff, eps2, margin2, w_i, w_k, (size_t)k)) return -1;
        std::vector<uint8_t> take(nb, 0);
        int still = 0;
        for (int j = 0; j < nb; j++) {
            if (!open_q[j]) continue;
            if (margin_h[j] > 0.0f || (size_t)kg_eff >= n_groups) { take[j] = 1; open_q[j] = 0; } else still++;
        }
        MSE_HIP_TRY(hipMemcpyAsync(take_dev, take.data(), (size_t)nb, hipMemcpyHostToDevice, st));
        if (launch_scatter_rows4(idx_dev, take_dev, nb, k, w_i, out_ids, out_stride, st) ||
            launch_scatter_rows4(idx_dev, take_dev, nb, k, w_k, out_keys, out_stride, st)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(st));
        if (still == 0) return 0;
        if (kg_eff >= TOPK_KMAX) break;
        kg = kg_eff * 4;
    }
    for (int j = 0; j < nb; j++) {   // cannot widen further: the exact pass, straight into the query's own output rows
        if (!open_q[j]) continue;
        if (index_pass_exact(idx, wq32 + (size_t)j * d, 1, k, out_ids + (size_t)bad[j] * out_stride, out_keys + (size_t)bad[j] * out_stride,
                             out_stride, f)) return -1;
    }
    return 0;
}

// The grouped search over the `total` gathered queries (idx->q32), k results each into ids_dev / keys_dev [total][k]: the sequence of
// bruteforce.hip grouped_topk_dev on f32 keys.  The exact regime holds every distance, so it takes the dense path at once; the
// matrix-core regime runs the rounds of the prefix path (grouped_prefix_drive) and sends what they leave to the dense path.
int index_run_grouped(mse_index* idx, const mse_groups* g, const mse_filter* f, size_t total, int k, bool mfma, uint32_t* ids_dev, float* keys_dev) {
    mse_searcher* s = idx->scratch;
    hipStream_t st = s->stream;
    const size_t d = idx->d;
    const float* q32 = idx->q32.as<float>();
    const size_t dtile = (size_t)dense_pass_queries(g->n_rows, 8);
    s->last_grouped[0] = s->last_grouped[1] = s->last_grouped[2] = 0;
    if (!mfma) {
        for (size_t q0 = 0; q0 < total; q0 += dtile) {
            const int m = (int)std::min(dtile, total - q0);
            if (index_pass_exact(idx, q32 + q0 * d, m, k, ids_dev + q0 * k, keys_dev + q0 * k, (size_t)k, f, g)) return -1;
        }
        s->last_grouped[2] = (uint32_t)total;
        return 0;
    }
    const size_t tile = (size_t)mfma_query_tile((int)d);
    auto round = [&](const void* qv, size_t nq, size_t kp, const std::vector<uint32_t>* dst, std::vector<uint32_t>* open,
                     std::vector<uint32_t>* reps) -> int {
        const float* qs = reinterpret_cast<const float*>(qv);
        if (s->grp_ids.ensure(nq * kp * 4) || s->grp_keys.ensure(nq * kp * 4)) return -1;
        for (size_t q0 = 0; q0 < nq; q0 += tile) {
            const int m = (int)std::min(tile, nq - q0);
            if (index_pass_mfma(idx, qs + q0 * d, m, (int)kp, s->grp_ids.as<uint32_t>() + q0 * kp, s->grp_keys.as<float>() + q0 * kp, kp, f)) return -1;
        }
        return grouped_collapse_round(s, g, 4, nq, kp, k, 0, dst, keys_dev, ids_dev, (size_t)k, open, reps);
    };
    auto dense = [&](const void* qv, size_t nr, const std::vector<uint32_t>& dst) -> int {
        const float* qs = reinterpret_cast<const float*>(qv);
        if (s->grp_idx.ensure(8 * 4)) return -1;
        for (size_t q0 = 0; q0 < nr; q0 += dtile) {
            const int m = (int)std::min(dtile, nr - q0);
            MSE_HIP_TRY(hipMemcpyAsync(s->grp_idx.p, dst.data() + q0, (size_t)m * 4, hipMemcpyHostToDevice, st));
            if (index_pass_exact(idx, qs + q0 * d, m, k, ids_dev, keys_dev, (size_t)k, f, g, s->grp_idx.as<uint32_t>())) return -1;
            MSE_HIP_TRY(hipStreamSynchronize(st));   // the indices are replaced by the next pass
        }
        return 0;
    };
    return grouped_prefix_drive(s, q32, d * 4, total, (size_t)k, round, dense);
}

// one engine call for a group of requests (worker thread; every caller of the group holds the shared lock)
int index_run_group(mse_index* idx, DispatchReq* const* reqs, size_t n_req) {
    mse_searcher* s = idx->scratch;
    hipStream_t st = s->stream;
    const size_t d = idx->d, n = idx->n;
    size_t total = 0, kmax = 0;
    for (size_t i = 0; i < n_req; i++) { total += reqs[i]->nq; kmax = std::max(kmax, reqs[i]->k); }
    const mse_filter* f = static_cast<const mse_filter*>(reqs[0]->aux0);   // the group's filter (its key, index_run_batch), or null
    const mse_groups* grp = static_cast<const mse_groups*>(reqs[0]->aux1);   // ... and its grouping, or null
    if (total == 0 || kmax == 0 || n == 0 || (f && f->count == 0)) return 0;   // outputs were pre-filled with "nothing found"
    const size_t in_bytes = total * d * 4, out_bytes = total * kmax * 8;
    if (idx->pin.ensure(std::max(in_bytes, out_bytes), (size_t)1 << 20)) return -1;
    if (idx->q32.ensure(in_bytes) || idx->out.ensure(out_bytes)) return -1;
    char* p = idx->pin.as<char>();
    for (size_t i = 0, o = 0; i < n_req; i++) { memcpy(p + o, reqs[i]->queries, reqs[i]->nq * d * 4); o += reqs[i]->nq * d * 4; }
    MSE_HIP_TRY(hipMemcpyAsync(idx->q32.p, idx->pin.p, in_bytes, hipMemcpyHostToDevice, st));
    uint32_t* ids_dev = idx->out.as<uint32_t>();
    float* keys_dev = reinterpret_cast<float*>(idx->out.as<char>() + total * kmax * 4);
    s->last_widened = 0; s->last_max_groups = 0;
    // same rule as the f16 dispatcher (dispatch.hip): the matrix-core pass for more than 8 queries, and for any count once the
    // rows have outgrown the caches
    // (filtered: the id-list pass on the sparse side of the crossover, bruteforce.hip filter_sparse)
    const bool mfma = (total > 8 || n >= ((size_t)1 << 22)) && !(f && filter_sparse(&idx->view, f, total));
    const size_t tile = mfma ? (size_t)mfma_query_tile((int)d) : 8;
    if (grp && index_run_grouped(idx, grp, f, total, (int)kmax, mfma, ids_dev, keys_dev)) return -1;
    for (size_t q0 = 0; !grp && q0 < total; q0 += tile) {
        const int m = (int)std::min(tile, total - q0);
        const int rc = mfma ? index_pass_mfma(idx, idx->q32.as<float>() + q0 * d, m, (int)kmax, ids_dev + q0 * kmax, keys_dev + q0 * kmax, kmax, f)
                            : index_pass_exact(idx, idx->q32.as<float>() + q0 * d, m, (int)kmax, ids_dev + q0 * kmax, keys_dev + q0 * kmax, kmax, f);
        if (rc) return -1;
    }
    MSE_HIP_TRY(hipMemcpyAsync(idx->pin.p, idx->out.p, out_bytes, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    const uint32_t* ids_h = reinterpret_cast<const uint32_t*>(p);
    const float* keys_h = reinterpret_cast<const float*>(p + total * kmax * 4);
    for (size_t i = 0, row = 0; i < n_req; i++) {
        DispatchReq* r = reqs[i];
        float* dist = static_cast<float*>(r->out_a);
        int64_t* lab = static_cast<int64_t*>(r->out_b);
        for (size_t q = 0; q < r->nq; q++, row++)
            for (size_t j = 0; j < r->k; j++) {
                const uint32_t id = ids_h[row * kmax + j];
                if (id == ID_NONE) continue;
                dist[q * r->k + j] = keys_h[row * kmax + j];
                lab[q * r->k + j] = (int64_t)id;
            }
    }
    return 0;
}

void index_run_batch(mse_index* idx, std::vector<DispatchReq*>& batch) {
    auto run = [idx](std::vector<DispatchReq*>& group) {
        idx->retried_alone += run_shared(group, [idx](DispatchReq* const* reqs, size_t n) { return index_run_group(idx, reqs, n); });
    };
    bool filtered = false;
    for (const DispatchReq* r : batch) filtered = filtered || r->aux0 || r->aux1;
    if (!filtered) { run(batch); return; }   // unfiltered, ungrouped requests only: one group, as always
    // requests share a pass only with requests of the same filter object (null = unfiltered) and the same grouping object (null = ungrouped)
    for_each_shared_group(batch, [](const DispatchReq& a, const DispatchReq& b) { return a.aux0 == b.aux0 && a.aux1 == b.aux1; }, run);
}

}  // namespace

static int index_search(mse_index* idx, const mse_filter* f, const float* queries, size_t nq, size_t k, float* distances, int64_t* labels,
                        const mse_groups* g = nullptr) {
    if (!idx) return fail("null index");
    if (nq == 0 || k == 0) return 0;
    if (!queries || !distances || !labels) return fail("null argument");
    if (k > (size_t)TOPK_KMAX - 64) return fail("k too large (max 1984)");
    // index.read() of src/main.rs:1046: any number of searches at once; they meet in the coalescer and share passes (a filtered one
    // with the searches of the same filter object: DispatchReq::aux0 is the group key)
    idx->rw.lock_shared();
    if (f && check_filter(&idx->view, f)) { idx->rw.unlock_shared(); return -1; }   // rows past the filter are excluded; add only grows
    if (g && check_groups(&idx->view, g)) { idx->rw.unlock_shared(); return -1; }   // rows past the grouping are groups of their own
    for (size_t i = 0; i < nq * k; i++) { distances[i] = -FLT_MAX; labels[i] = -1; }
    DispatchReq r;
    r.queries = queries; r.nq = nq; r.k = k; r.out_a = distances; r.out_b = labels; r.aux0 = f; r.aux1 = g;
    const int rc = idx->co->submit(r);
    idx->rw.unlock_shared();
    return rc;
}

mse_index* mse_index_new(int d) {
    if (d <= 0 || d % 64 != 0 || d > D_MAX) {
        fail("index width must be a positive multiple of 64");
        return nullptr;
    }
    mse_index* idx = new (std::nothrow) mse_index();
    if (!idx) { fail("out of host memory"); return nullptr; }
    idx->d = d;
    if (hipGetDevice(&idx->device) != hipSuccess) idx->device = 0;
    idx->scratch = scratch_searcher_new();
    if (!idx->scratch) { delete idx; return nullptr; }
    idx->view.d = d; idx->view.owned = false; idx->view.n_cu = idx->scratch->n_cu; idx->view.device = idx->device;
    if (hipMalloc((void**)&idx->view.norm_bits_dev, 12) != hipSuccess || hipMemset(idx->view.norm_bits_dev, 0, 12) != hipSuccess) {
        mse_index_free(idx);
        fail("device allocation failed for the index");
        return nullptr;
    }
    idx->view.norm_ready = true;   // kept current by add()
    idx->scratch->base = &idx->view;
    const int device = idx->device;
    // at most one matrix-core pass worth of queries per gather; the wait budget follows the row count (add)
    idx->co.reset(new Coalescer((size_t)mfma_query_tile((int)idx->view.d), 200, [idx](std::vector<DispatchReq*>& b) { index_run_batch(idx, b); },
                                [device] { (void)hipSetDevice(device); }));
    return idx;
}
void mse_index_free(mse_index* idx) {
    if (!idx) return;
    idx->co.reset();   // joins the worker
    if (idx->scratch) mse_searcher_free(idx->scratch);
    if (idx->codes) (void)hipFree(idx->codes);
    if (idx->view.norm_bits_dev) (void)hipFree(idx->view.norm_bits_dev);
    delete idx;
}
size_t mse_index_ntotal(const mse_index* idx) { return idx ? idx->n : 0; }

int mse_index_add(mse_index* idx, const float* x, size_t n) {
    if (!idx) return fail("null index");
    if (n == 0) return 0;
    std::lock_guard<SharedExclusive> g(idx->rw);   // index.write() of src/main.rs:1016: waits for the searches in flight, holds new ones off
    const size_t d = idx->d;
    hipStream_t st = idx->scratch->stream;
    if (idx->n + n > 0xFFFFFFFEull) return fail("index full");
    if (idx->n + n > idx->cap) {
        size_t ncap = std::max<size_t>(idx->cap * 2, idx->n + n);
        ncap = std::max<size_t>(ncap, 1024);
        uint16_t* np = nullptr;
        MSE_HIP_TRY(hipMalloc((void**)&np, ncap * d * 2));
        hipError_t ce = idx->n ? hipMemcpyAsync(np, idx->codes, idx->n * d * 2, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (ce == hipSuccess) ce = hipStreamSynchronize(st);
        if (ce != hipSuccess) {   // the old block stays in place; the new one must not leak
            (void)hipFree(np);
            return fail(std::string("mse_index_add: growing the index failed: ") + hipGetErrorString(ce));
        }
        if (idx->codes) (void)hipFree(idx->codes);
        idx->codes = np;
        idx->cap = ncap;
    }
    // fp32 rows are staged on the device and narrowed there (RNE), as FAISS QT_fp16 encodes them
    DevBuf& stage = idx->scratch->misc;
    if (stage.ensure(n * d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(stage.p, x, n * d * 4, hipMemcpyHostToDevice, st));
    if (launch_f32_to_f16(stage.as<float>(), n * d, idx->codes + idx->n * d, st)) return -1;
    // the certificate's row-norm bound only ever grows: fold the new rows in (atomic maxima on the device)
    if (launch_row_norm_max(idx->codes + idx->n * d, n, (int)d, idx->view.norm_bits_dev, st)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(st));
    idx->n += n;
    idx->view.dev = idx->codes;
    idx->view.n = idx->n;
    idx->co->set_max_wait_us(default_wait_us(idx->n, d * 2));
    return 0;
}

int mse_index_search(mse_index* idx, const float* queries, size_t nq, size_t k, float* distances, int64_t* labels) {
    return index_search(idx, nullptr, queries, nq, k, distances, labels);
}

int mse_index_search_filtered(mse_index* idx, const mse_filter* f, const float* queries, size_t nq, size_t k, float* distances,
                              int64_t* labels) {
    if (!idx) return fail("null index");
    if (!f) return fail("null filter");
    return index_search(idx, f, queries, nq, k, distances, labels);
}

int mse_index_search_grouped(mse_index* idx, const mse_groups* g, const mse_filter* f, const float* queries, size_t nq, size_t k, float* distances,
                             int64_t* labels) {
    if (!idx) return fail("null index");
    if (!g) return fail("null grouping");
    return index_search(idx, f, queries, nq, k, distances, labels, g);
}

int mse_index_stats(mse_index* idx, uint64_t out[6]) {
    if (!idx || !out) return fail("null argument");
    const DispatchStats st = idx->co->stats();
    out[0] = st.queries; out[1] = st.requests; out[2] = st.passes; out[3] = st.max_pass_queries; out[4] = st.deadline_fires;
    out[5] = idx->retried_alone.load();
    return 0;
}

// ---- product quantiser ----------------------------------------------------------------------------
mse_pq* mse_pq_load(const float* centroids, size_t n_centroids, const float* transform, size_t n_dims,
                    size_t n_dims_per_code) {
    if (n_centroids == 0 || n_centroids > 256) { fail("at most 256 centroids (vector.rs:337)"); return nullptr; }
    if (n_dims == 0 || n_dims_per_code == 0 || n_dims % n_dims_per_code != 0) {
        fail("n_dims must be a positive multiple of n_dims_per_code");
        return nullptr;
    }
    if ((n_dims / n_dims_per_code) * n_centroids * 4 > 160 * 1024) { fail("PQ table exceeds LDS"); return nullptr; }
    mse_pq* pq = new (std::nothrow) mse_pq();
    if (!pq) { fail("out of host memory"); return nullptr; }
    pq->n_centroids = n_centroids; pq->d = n_dims; pq->dpc = n_dims_per_code; pq->n_chunks = n_dims / n_dims_per_code;
    if (hipGetDevice(&pq->device) != hipSuccess) pq->device = 0;
    if (hipMalloc((void**)&pq->centroids, n_centroids * n_dims * 4) != hipSuccess ||
        hipMalloc((void**)&pq->transform, n_dims * n_dims * 4) != hipSuccess ||
        hipMemcpy(pq->centroids, centroids, n_centroids * n_dims * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(pq->transform, transform, n_dims * n_dims * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void**)&pq->transform_t, n_dims * n_dims * 4) != hipSuccess) {
        mse_pq_free(pq);
        fail("device allocation/copy failed for the quantiser");
        return nullptr;
    }
    {
        std::vector<float> tt(n_dims * n_dims);
        for (size_t i = 0; i < n_dims; i++)
            for (size_t k = 0; k < n_dims; k++) tt[k * n_dims + i] = transform[i * n_dims + k];
        if (hipMemcpy(pq->transform_t, tt.data(), n_dims * n_dims * 4, hipMemcpyHostToDevice) != hipSuccess) {
            mse_pq_free(pq);
            fail("device copy failed for the quantiser");
            return nullptr;
        }
    }
    return pq;
}
void mse_pq_free(mse_pq* pq) {
    if (!pq) return;
    delete pq->co;   // joins its worker
    pq->co = nullptr;
    if (pq->centroids) (void)hipFree(pq->centroids);
    if (pq->transform) (void)hipFree(pq->transform);
    if (pq->transform_t) (void)hipFree(pq->transform_t);
    if (pq->scratch) mse_searcher_free(pq->scratch);
    if (pq->lane2) mse_searcher_free(pq->lane2);
    if (pq->lane3) mse_searcher_free(pq->lane3);
    delete pq;
}

int mse_pq_apply_transform(mse_pq* pq, const float* x, size_t n, float* out) {
    if (!pq) return fail("null quantiser");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    const size_t bytes = n * pq->d * 4;
    if (pq->a.ensure(bytes) || pq->b.ensure(bytes)) return -1;
    MSE_HIP_TRY(hipMemcpy(pq->a.p, x, bytes, hipMemcpyHostToDevice));
    if (launch_pq_transform(pq->transform, (int)pq->d, pq->a.as<float>(), n, pq->b.as<float>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, pq->b.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int mse_pq_quantize_batch(mse_pq* pq, const float* x, size_t n, uint8_t* codes) {
    if (!pq) return fail("null quantiser");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    const size_t bytes = n * pq->d * 4;
    if (pq->a.ensure(bytes) || pq->b.ensure(bytes) || pq->c.ensure(n * pq->n_chunks)) return -1;
    MSE_HIP_TRY(hipMemcpy(pq->a.p, x, bytes, hipMemcpyHostToDevice));
    if (launch_pq_transform(pq->transform, (int)pq->d, pq->a.as<float>(), n, pq->b.as<float>(), nullptr)) return -1;
    if (launch_pq_quantize(pq->centroids, (int)pq->n_centroids, (int)pq->d, (int)pq->dpc, pq->b.as<float>(), n,
                           pq->c.as<uint8_t>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(codes, pq->c.p, n * pq->n_chunks, hipMemcpyDeviceToHost));
    return 0;
}

// device LUT build into pq->c (needs pq->mu held); query_dev = fp32 [d] on device
static int build_lut_locked(mse_pq* pq, const float* query_dev, hipStream_t st) {
    if (pq->b.ensure(pq->d * 4) || pq->c.ensure(pq->n_chunks * pq->n_centroids * 4)) return -1;
    if (launch_pq_transform_vec(pq->transform_t, (int)pq->d, query_dev, pq->b.as<float>(), st)) return -1;
    return launch_pq_lut(pq->centroids, (int)pq->n_centroids, (int)pq->d, (int)pq->dpc, pq->b.as<float>(),
                         pq->c.as<float>(), st);
}

int mse_pq_preprocess_query(mse_pq* pq, const float* query, float* lut) {
    if (!pq) return fail("null quantiser");
    std::lock_guard<std::mutex> g(pq->mu);
    if (pq->a.ensure(pq->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(pq->a.p, query, pq->d * 4, hipMemcpyHostToDevice));
    if (build_lut_locked(pq, pq->a.as<float>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(lut, pq->c.p, pq->n_chunks * pq->n_centroids * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_pq_adc(mse_pq* pq, const float* lut, const uint8_t* codes, size_t n, int64_t* out) {
    if (!pq) return fail("null quantiser");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    const size_t lut_bytes = pq->n_chunks * pq->n_centroids * 4;
    // + 4 KiB of slack: the full-scan kernel fetches whole groups of 64 vectors (pq.hip)
    if (pq->a.ensure(lut_bytes) || pq->b.ensure(n * pq->n_chunks + 4096) || pq->c.ensure(n * 8)) return -1;
    MSE_HIP_TRY(hipMemcpy(pq->a.p, lut, lut_bytes, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(pq->b.p, codes, n * pq->n_chunks, hipMemcpyHostToDevice));
    if (launch_pq_adc(pq->a.as<float>(), (int)pq->n_chunks, (int)pq->n_centroids, pq->b.as<uint8_t>(), n, nullptr, n,
                      nullptr, 0, nullptr, pq->c.as<int64_t>(), device_cu_count(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, pq->c.p, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

mse_codes* mse_codes_from_host(const uint8_t* codes, size_t n, size_t code_size, const uint8_t* descriptors,
                               size_t n_descriptors) {
    if (code_size == 0) { fail("code_size must be positive"); return nullptr; }
    mse_codes* c = new (std::nothrow) mse_codes();
    if (!c) { fail("out of host memory"); return nullptr; }
    c->n = n; c->code_size = code_size; c->n_desc = descriptors ? n_descriptors : 0;
    // + 4 KiB / 256 B of slack: the full-scan kernel fetches whole groups of 64 vectors (pq.hip)
    bool ok = hipMalloc((void**)&c->codes, n * code_size + 4096) == hipSuccess;
    if (ok && n) ok = hipMemcpy(c->codes, codes, n * code_size, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && c->n_desc) {
        ok = hipMalloc((void**)&c->desc, n * c->n_desc + 256) == hipSuccess;
        if (ok && n) ok = hipMemcpy(c->desc, descriptors, n * c->n_desc, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { mse_codes_free(c); fail("device allocation/copy failed for PQ codes"); return nullptr; }
    return c;
}
void mse_codes_free(mse_codes* c) {
    if (!c) return;
    if (c->codes) (void)hipFree(c->codes);
    if (c->desc) (void)hipFree(c->desc);
    delete c;
}
size_t mse_codes_len(const mse_codes* c) { return c ? c->n : 0; }

int mse_pq_adc_gather(mse_pq* pq, const mse_codes* c, const float* lut, const float* scales, const uint32_t* ids,
                      size_t n_ids, int64_t* out) {
    if (!pq || !c) return fail("null quantiser or codes");
    if (c->code_size != pq->n_chunks) return fail("code size does not match the quantiser");
    if (n_ids == 0) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    const size_t lut_bytes = pq->n_chunks * pq->n_centroids * 4;
    const size_t sc_bytes = c->n_desc * 4;
    if (pq->a.ensure(lut_bytes + 256 + sc_bytes) || pq->b.ensure(n_ids * 4) || pq->c.ensure(n_ids * 8)) return -1;
    float* scales_dev = nullptr;
    MSE_HIP_TRY(hipMemcpy(pq->a.p, lut, lut_bytes, hipMemcpyHostToDevice));
    if (scales && c->n_desc) {
        scales_dev = reinterpret_cast<float*>(pq->a.as<char>() + ((lut_bytes + 255) & ~(size_t)255));
        MSE_HIP_TRY(hipMemcpy(scales_dev, scales, sc_bytes, hipMemcpyHostToDevice));
    }
    MSE_HIP_TRY(hipMemcpy(pq->b.p, ids, n_ids * 4, hipMemcpyHostToDevice));
    if (launch_pq_adc(pq->a.as<float>(), (int)pq->n_chunks, (int)pq->n_centroids, c->codes, c->n, pq->b.as<uint32_t>(),
                      n_ids, scales_dev ? c->desc : nullptr, (int)c->n_desc, scales_dev, pq->c.as<int64_t>(),
                      device_cu_count(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, pq->c.p, n_ids * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ---- the flat ADC scan (mse_pq_scan_topk and its batch, block and filtered forms) ----
namespace mse {

int check_pq_mode(int mode) {
    if (mode != MSE_PQ_FILTER_AUTO && mode != MSE_PQ_FILTER_SCAN && mode != MSE_PQ_FILTER_LIST) return fail("unknown mode");
    return 0;
}
int check_pq_r(size_t r, size_t k) {
    if (std::max(r, k) > (size_t)TOPK_KMAX - 64) return fail("r too large (max 1984)");
    return 0;
}
static int check_pq_filter(const mse_pq* pq, const mse_codes* c, const mse_filter* f) {   // (also the debug hooks')
    if (!f) return fail("null filter");
    if (f->n_rows > c->n) return fail("filter is longer than the codes (" + std::to_string(f->n_rows) + " > " + std::to_string(c->n) + " rows)");
    if (f->device != pq->device) return fail("filter was made on another device than the quantiser's");   // no silent copy
    return 0;
}
int check_pq_scan(const mse_pq* pq, const mse_codes* c, const mse_searcher* s, size_t nq, size_t r, size_t k, const PqFilterArg* fa) {
    if (!pq || !c) return fail("null quantiser or codes");
    if (fa && (check_pq_filter(pq, c, fa->f) || check_pq_mode(fa->mode))) return -1;
    if (c->code_size != pq->n_chunks) return fail("code size does not match the quantiser");
    if (!fa && (nq == 0 || k == 0)) return 0;   // an unfiltered call with nothing to do is answered before r and the base are looked at
    if (check_pq_r(r, k)) return -1;
    if (s && s->base && s->base->n != c->n) return fail("base and codes differ in length");
    if (s && s->base && s->base->d != pq->d) return fail("base width differs from the quantiser");
    return 0;
}

int exact_rescore(const mse_base* b, const mse_codes* c, const float* scales_dev, const void* q16, const uint32_t* ids, size_t n, size_t per_query,
                  int64_t* out, hipStream_t st) {
    if (launch_score_rows(b->dev, b->n, (int)b->d, q16, false, ids, n, per_query, out, nullptr, st)) return -1;
    if (scales_dev && c->n_desc && launch_add_descriptor(ids, n, c->desc, (int)c->n_desc, c->n, scales_dev, out, st)) return -1;
    return 0;
}

}  // namespace mse

namespace {

int prep_table(mse_pq* pq, mse_searcher* s, const float* query_dev, float* t_dev, float* lut_dev) {
    if (launch_pq_transform_vec(pq->transform_t, (int)pq->d, query_dev, t_dev, s->stream)) return -1;
    return launch_pq_lut(pq->centroids, (int)pq->n_centroids, (int)pq->d, (int)pq->dpc, t_dev, lut_dev, s->stream);
}

// one lane of a batched scan: a searcher (its stream and scratch) and the lane's own transformed queries, tables and f16 queries
struct ScanLane { mse_searcher* s; float* t; float* lut; uint16_t* qf16; };

// what the steps of one scan call share
struct ScanRun {
    mse_pq* pq;
    const mse_codes* c;
    const PqFilterArg* fa;               // a filtered call's filter and mode, or null
    size_t nq, r, k;
    const float *queries_f32, *scales;   // host [nq][d]; host [n_desc] or null
    // the destination: a packed block on the device (a sharded scan's hand-over: launch_block_finish, topk.hip; ids lifted by
    // id_offset), or the caller's host arrays
    void* block_dev; uint64_t id_offset; int64_t* scores; uint32_t* ids;
    // filled by the steps
    const mse_filter* f = nullptr;       // the allowed rows (null: all) ...
    bool list = false;                   // ... and the resolved mode: LIST makes no pass over the codes (ADC over the filter's id list)
    const uint32_t* mask = nullptr;      // f's bitmap words for the masked scans and the masked expansion (null: unfiltered kernels)
    size_t mask_words = 0;
    const float *queries_dev = nullptr, *scales_dev = nullptr;   // scales_dev: null unless scales AND descriptors are there
    const uint8_t* desc = nullptr;       // the codes' descriptors when scales_dev, else null
    // batches of 4 .. 2048 queries: all transformed queries (pq->b) and tables (pq->c) up front, in two launches (the same kernels the
    // codec's batch entry points use; same arithmetic as the one-vector forms) instead of two small launches per query in front of every scan
    bool prep_all = false;
    ScanLane lanes[3] = {};
    int n_lanes = 1;
    bool four_ok = false, eight_ok = false;   // the nomination scans this call may use (scan_group_size)
    size_t n_in_eight = 0;                    // the call's first n_in_eight queries went through eight-per-pass groups
    int64_t* out_scores_dev = nullptr; uint32_t* out_ids_dev = nullptr;   // [nq][k] each
    int* flags_dev = nullptr;                 // [nq], non-zero = certified / exact
};

// n consecutive queries from q0 on, sharing one pass over the codes, on lane `lane`
struct ScanGroup { int lane; size_t q0; int n; };

// a group's tables: inside the call's array when that was built up front, else built here in the lane's scratch; null: failed
const float* group_tables(const ScanRun& run, const ScanGroup& g) {
    const ScanLane& ln = run.lanes[g.lane];
    const size_t d = run.pq->d, lut_floats = run.pq->n_chunks * run.pq->n_centroids;
    if (run.prep_all) return run.pq->c.as<float>() + g.q0 * lut_floats;
    for (int j = 0; j < g.n; j++)
        if (prep_table(run.pq, ln.s, run.queries_dev + (g.q0 + j) * d, ln.t + j * d, ln.lut + j * lut_floats)) return nullptr;
    return ln.lut;
}

// where level 0 of a tail's tournament comes from:
//   GROUPS_EXACT      the exact scans' maxima (i64, one per 64 vectors): the n_sel = min(r, n_groups) best groups, all of them expanded
//   GROUPS_NOMINATED  the integer scan's maxima (u32, group-major): n_nom groups expanded, one more selected only for its key
//   ID_LIST           no scan -- LIST mode, and every codec shape without a group-maximum scan under a filter: the ADC scores of the
//                     filter's ascending id list, the tournament over list positions (which order as their ids do)
//   ALL_ROWS          codec shapes without a group-maximum scan: every vector's ADC score
struct TailSource {
    enum Kind { GROUPS_EXACT, GROUPS_NOMINATED, ID_LIST, ALL_ROWS } kind;
    LevelRef l0;            // GROUPS_*: the scan's maxima (the other two take their scores in the tail, into s->scores)
    size_t n_sel, n_nom;    // GROUPS_*: groups the tournament selects / of those, expanded into candidates
    const Pq4Params* params;   // GROUPS_NOMINATED: the certificate's parameters
};

// Everything after the scan for the Q = g.n queries of a group, as ONE chain of launches with a query dimension (the kernels are
// latency-bound: four chains in a row cost more than the scan): the r best by ADC score -- from the candidates of the selected groups,
// re-scored by the gather kernel in the reference's arithmetic, or straight from the tournament over a list's scores -- then, for
// GROUPS_NOMINATED, the certificate flag (1 = provably the exact top-r of all vectors; 0 asks the caller to repeat the query through
// the exact scan), then with base vectors the exact fast_dot re-score of those r (+ descriptor bias) and the top k.  Under a filter the
// disallowed vectors of the selected groups are dropped at the expansion (a dropped vector is ID_NONE: the gather kernel scores it
// INT64_MIN and the select skips it).
// The buffers of the lane's searcher, every one at its final size for the whole group before the first launch that uses any of them
// (an ensure that grows frees the old allocation):
//   gkeys        the selected groups' keys [Q][n_sel] until the certificate has read them; then the final top-k's keys [Q][k]
//   cand_ids     the candidates [Q][n_nom * 64]
//   cand_scores  their ADC scores; once the top-r select has read them, the exact scores [Q][r]
//   out_ids      GROUPS_*: the top-r ids [Q][r] (a list's top-r ids stay where the tournament leaves them)
//   sel_keys     the top-r ADC scores [Q][r]
//   misc         the final top-k's ids [Q][k]
//   scores       ID_LIST / ALL_ROWS: the list's ADC scores
// Neither s->gmax nor, for GROUPS_*, s->scores is written: in a pair they hold query 1's and query 0's maxima until each one's own
// tournament has read them, and in the nomination route s->gmax holds all Q queries' maxima until theirs has.
// lut: the group's Q tables (a pair's second query makes a group of its own for its tail, with the pair's second table)
int scan_tail(const ScanRun& run, const ScanGroup& g, const float* lut, const TailSource& src) {
    const mse_pq* pq = run.pq;
    const mse_codes* c = run.c;
    const mse_filter* f = run.f;
    mse_searcher* s = run.lanes[g.lane].s;
    hipStream_t st = s->stream;
    const size_t d = pq->d, r = run.r, k = run.k, Q = (size_t)g.n;
    const bool groups = src.kind == TailSource::GROUPS_EXACT || src.kind == TailSource::GROUPS_NOMINATED;
    const size_t n_cand = src.n_nom * 64, n_sel = src.n_sel;   // (both 0 without groups)
    const uint32_t* list = src.kind == TailSource::ID_LIST ? f->ids : nullptr;
    const size_t n_list = list ? f->count : c->n;   // (a filter's count is > 0 here: an empty filter is answered without a launch)
    if (s->gkeys.ensure(Q * std::max(k, n_sel) * 8) || s->cand_ids.ensure(Q * n_cand * 4) || s->cand_scores.ensure(Q * std::max(r, n_cand) * 8) ||
        s->out_ids.ensure(Q * r * 4) || s->sel_keys.ensure(Q * r * 8) || s->misc.ensure(Q * k * 4) || (!groups && s->scores.ensure(n_list * 8)))
        return -1;
    const uint32_t* top_ids = nullptr;                      // the r best by ADC score [Q][r] ...
    const int64_t* top_scores = s->sel_keys.as<int64_t>();  // ... and their scores
    size_t top_stride = r;
    if (groups) {
#ifdef MSE_DEV_KERNELS
        // developer library, MSE_PQ_TAIL_SKIP=mask: the nomination scan WITHOUT stages of its tail (answers are garbage, every query is
        // reported certified): what the tail costs the scans that run beside it.  1 tournament, 2 expand + re-score, 4 exact top-r,
        // 8 certificate (and with any bit: nothing after the certificate either)
        static const int tail_skip = getenv("MSE_PQ_TAIL_SKIP") ? atoi(getenv("MSE_PQ_TAIL_SKIP")) : 0;
        const int skip = src.kind == TailSource::GROUPS_NOMINATED ? tail_skip : 0;
#else
        const int skip = 0;
#endif
        uint32_t* gsel = nullptr;                           // [Q][n_sel]
        if (!(skip & 1) && descend(s, src.l0, (int)Q, (int)n_sel, &gsel, s->gkeys.p)) return -1;
        if (!(skip & 2) && gsel) {
            if (f ? launch_expand_groups_masked(gsel, n_sel, src.n_nom, 64, c->n, run.mask, run.mask_words, s->cand_ids.as<uint32_t>(), n_cand, (int)Q, st)
                  : launch_expand_groups(gsel, n_sel, src.n_nom, 64, c->n, s->cand_ids.as<uint32_t>(), n_cand, (int)Q, st)) return -1;
            if (launch_pq_adc(lut, (int)pq->n_chunks, (int)pq->n_centroids, c->codes, c->n, s->cand_ids.as<uint32_t>(), n_cand, run.desc,
                              (int)c->n_desc, run.scales_dev, s->cand_scores.as<int64_t>(), s->n_cu, st, (int)Q, Q > 1 ? n_cand : 0)) return -1;
        }
        if (!(skip & 4)) {
            SelectArgs a{};
            a.kind = KEY_I64; a.list_ids = s->cand_ids.as<uint32_t>(); a.list_keys = s->cand_scores.p; a.list_stride = n_cand;
            a.n_list = n_cand; a.k = (int)r; a.out_ids = s->out_ids.as<uint32_t>(); a.out_keys = s->sel_keys.p; a.out_stride = r; a.nq = (int)Q;
            // GROUPS_EXACT: r group maxima reach the r-th best group's key, so r vectors do: the key is a floor for the select.  This
            // leans on the scan kernels and pq_adc_kernel producing the SAME i64 for a vector (same adds in the same order, bias added
            // after the conversion); tests/test_gpu_pq_index_graph.py::test_group_maxima_equal_the_gathered_scores pins exactly that.
            // Under a filter the maxima are over ALLOWED vectors, so the argument holds as long as the r-th key belongs to a group with
            // an allowed vector.  When fewer than r groups have one, the r-th key is INT64_MIN, whose sortable form is 0: a floor of 0
            // cuts nothing, and padding (ID_NONE) is skipped by the select before the floor is looked at (topk.hip), so it is never
            // admitted.  (The integer maxima of GROUPS_NOMINATED are no floor for exact scores.)
            if (src.kind == TailSource::GROUPS_EXACT && n_sel == r) a.floor_hi = s->last_kth;
            if (launch_select(a, st)) return -1;
        }
        if (skip) {
            MSE_HIP_TRY(hipMemsetAsync(run.flags_dev + g.q0, 1, Q * sizeof(int), st));
            return 0;
        }
        top_ids = s->out_ids.as<uint32_t>();
        // the vectors that must exist among the nominated: min(r, rows) -- under a filter min(r, allowed rows).  The bound from the best
        // excluded group stays sound there: its masked maximum bounds every ALLOWED vector outside the nominated groups, and a masked
        // vector's key (the all-zero sum) is the smallest possible
        if (src.kind == TailSource::GROUPS_NOMINATED &&
            launch_pq4_certify(src.params, s->gkeys.as<uint32_t>(), (int)src.n_nom, (int)n_sel, top_ids, top_scores, r,
                               (int)std::min(r, f ? f->count : c->n), (int)Q, run.flags_dev + g.q0, st)) return -1;
    } else {
        if (launch_pq_adc(lut, (int)pq->n_chunks, (int)pq->n_centroids, c->codes, c->n, list, n_list, run.desc, (int)c->n_desc, run.scales_dev,
                          s->scores.as<int64_t>(), s->n_cu, st)) return -1;
        LevelRef l0{KEY_I64, s->scores.p, n_list, 1, n_list, false, 0};
        uint32_t* sel = nullptr;
        if (descend(s, l0, 1, (int)r, &sel, s->sel_keys.p)) return -1;
        if (list && launch_map_positions(sel, r, list, st)) return -1;
        top_ids = sel;
    }
    if (s->base) {
        // exact re-score: f16(query) . base[id] (+ descriptor bias), query_disk_index.rs:168-170,477 -- the group's queries per launch
        uint16_t* qf16 = run.lanes[g.lane].qf16;
        if (launch_f32_to_f16(run.queries_dev + g.q0 * d, Q * d, qf16, st)) return -1;
        if (exact_rescore(s->base, c, run.scales_dev, qf16, top_ids, Q * r, r, s->cand_scores.as<int64_t>(), st)) return -1;
        SelectArgs a{};
        a.kind = KEY_I64; a.list_ids = top_ids; a.list_keys = s->cand_scores.p; a.list_stride = r; a.n_list = r;
        a.k = (int)k; a.out_ids = s->misc.as<uint32_t>(); a.out_keys = s->gkeys.p; a.out_stride = k; a.nq = (int)Q;
        if (launch_select(a, st)) return -1;
        top_ids = s->misc.as<uint32_t>();
        top_scores = s->gkeys.as<int64_t>();
        top_stride = k;
    }
    uint32_t* const out_ids = run.out_ids_dev + g.q0 * k;
    int64_t* const out_scores = run.out_scores_dev + g.q0 * k;
    if (Q == 1) {   // (one row: the plain copies the one-query tail always made, not the strided copy's kernel)
        MSE_HIP_TRY(hipMemcpyAsync(out_ids, top_ids, k * 4, hipMemcpyDeviceToDevice, st));
        MSE_HIP_TRY(hipMemcpyAsync(out_scores, top_scores, k * 8, hipMemcpyDeviceToDevice, st));
    } else {
        MSE_HIP_TRY(hipMemcpy2DAsync(out_ids, k * 4, top_ids, top_stride * 4, k * 4, Q, hipMemcpyDeviceToDevice, st));
        MSE_HIP_TRY(hipMemcpy2DAsync(out_scores, k * 8, top_scores, top_stride * 8, k * 8, Q, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

// One query or a PAIR of the flat ADC scan, exact, entirely on the lane's stream (no host synchronisation):
//   table(query) -> scan of all codes keeping one maximum per 64 vectors (a pair shares ONE pass over the codes: pq_scan64x2_kernel)
//   -> per query its own tail (two Q = 1 chains for a pair)
// LIST mode and codec shapes without a group-maximum scan make no pass: their tails score the filter's id list, or every vector.
int scan_exact_group(const ScanRun& run, const ScanGroup& g) {
    const mse_pq* pq = run.pq;
    const mse_codes* c = run.c;
    mse_searcher* s = run.lanes[g.lane].s;
    const size_t lut_floats = pq->n_chunks * pq->n_centroids, n_groups = (c->n + 63) / 64;
    const bool gm = !run.list && pq_scan_gmax_supported((int)pq->n_chunks, (int)pq->n_centroids, run.desc, (int)c->n_desc, run.scales_dev);
    const float* lut = group_tables(run, g);
    if (!lut) return -1;
    // a pair: query 0's maxima in s->scores, query 1's in s->gmax
    int64_t* gmax[2] = {nullptr, nullptr};
    if (gm) {
        if (s->scores.ensure(n_groups * 8) || (g.n == 2 && s->gmax.ensure(n_groups * 8))) return -1;
        gmax[0] = s->scores.as<int64_t>();
        gmax[1] = s->gmax.as<int64_t>();
        if (g.n == 2 ? launch_pq_scan_gmax2(lut, lut + lut_floats, c->codes, c->n, run.desc, run.scales_dev, gmax[0], gmax[1], s->n_cu, s->stream,
                                            run.mask, run.mask_words)
                     : launch_pq_scan_gmax(lut, c->codes, c->n, run.desc, run.scales_dev, gmax[0], s->n_cu, s->stream, run.mask, run.mask_words))
            return -1;
    }
    const size_t rg = gm ? std::min(run.r, n_groups) : 0;
    for (int j = 0; j < g.n; j++) {
        TailSource src{gm ? TailSource::GROUPS_EXACT : run.f ? TailSource::ID_LIST : TailSource::ALL_ROWS,
                       LevelRef{KEY_I64, gmax[j], n_groups, 1, n_groups, false, 0}, rg, rg, nullptr};
        if (scan_tail(run, ScanGroup{g.lane, g.q0 + j, 1}, lut + j * lut_floats, src)) return -1;
    }
    return 0;
}

// the next event pair of the lane's pool (mse_pq_scan_timing: around the nomination scan's launch; read and returned by scan_drain_timing)
int scan_event_pair(mse_searcher* s, hipEvent_t te[2]) {
    while (s->ev_pool.size() < s->ev_used + 2) {
        hipEvent_t e = nullptr;
        MSE_HIP_TRY(hipEventCreate(&e));
        s->ev_pool.push_back(e);
    }
    te[0] = s->ev_pool[s->ev_used++];
    te[1] = s->ev_pool[s->ev_used++];
    return 0;
}

// How many groups to nominate: the certificate needs every group whose integer maximum lies within ~2 eps of the r-th exact
// score.  With 12-bit tables that is a few tens of vectors at 1e8 codes (r + max(64, r / 2) groups); the 8-bit step is 16 times
// coarser and the band holds ~0.7 r vectors on random codes (simulated at 1e7 codes, r = 200: 339 groups reach it): 2 r + 112.
size_t pq_nominated(size_t r, int NQ) { return NQ == 4 ? r + std::max<size_t>(64, r / 2) : 2 * r + 112; }

// FOUR (12-bit tables) or EIGHT (8-bit tables) queries in one pass over the codes (pq_scan64x4_kernel: integer nomination under a
// certificate, pq.hip), then ONE tail for all of them: per query the n_nom best groups by their integer maximum (+ one more, whose key
// bounds everything excluded) are re-scored, and flags_dev[q] = 0 asks the caller to repeat query q through the exact scan.
int scan_nominated_group(const ScanRun& run, const ScanGroup& g) {
    const mse_codes* c = run.c;
    mse_searcher* s = run.lanes[g.lane].s;
    hipStream_t st = s->stream;
    const int NQ = g.n;
    const float* lut = group_tables(run, g);
    if (!lut) return -1;
    const size_t n_groups = (c->n + 63) / 64;
    // one more group than nominated is selected, only for its key
    const size_t n_nom = std::min(n_groups, pq_nominated(run.r, NQ));
    const size_t n_sel = std::min(n_groups, n_nom + 1);
    if (n_sel > (size_t)TOPK_KMAX) return fail("pq scan: r too large for the four-query scan");
    if (s->pq4.ensure(pq4_table_bytes() + 8 * sizeof(Pq4Params)) || s->gmax.ensure((size_t)NQ * n_groups * 4)) return -1;
    void* table = s->pq4.p;
    Pq4Params* params = reinterpret_cast<Pq4Params*>(s->pq4.as<char>() + pq4_table_bytes());
    if (launch_pq4_table(lut, run.scales_dev, NQ, table, params, st, NQ)) return -1;
    hipEvent_t te[2] = {nullptr, nullptr};
    if (run.pq->timing) {
        if (scan_event_pair(s, te)) return -1;
        MSE_HIP_TRY(hipEventRecord(te[0], st));
    }
    if (launch_pq_scan_gmax4(table, c->codes, c->n, run.desc, s->gmax.as<uint32_t>(), s->n_cu, st, NQ, run.mask, run.mask_words)) return -1;
    if (te[1]) MSE_HIP_TRY(hipEventRecord(te[1], st));
    // group-major: element (q, g) at gmax[g * NQ + q]
    return scan_tail(run, g, lut, TailSource{TailSource::GROUPS_NOMINATED, LevelRef{KEY_U32, s->gmax.p, 1, (size_t)NQ, n_groups, false, 0}, n_sel, n_nom, params});
}

// queries go through in groups that share one pass over the codes: EIGHTS (8-bit tables) and FOURS (12-bit tables) -- integer
// nomination under a certificate, pq_scan64x4_kernel --, then a PAIR (pq_scan64x2_kernel, exact), then a single one.  (A filtered LIST
// call shares no pass over the codes: its queries go one by one.)  The size of the next group with `remaining` queries to go:
int scan_group_size(size_t remaining, bool eight_ok, bool four_ok, bool list) {
    return (eight_ok && remaining >= 8) ? 8 : (four_ok && remaining >= 4) ? 4 : (remaining >= 2 && !list) ? 2 : 1;
}

// the empty answer -- no codes, or a filter that allows no row: everything is padding and no scan is launched.  1: answered, 0: go on
int scan_answer_empty(const ScanRun& run) {
    const size_t n_out = run.nq * run.k;
    if (!run.block_dev)
        for (size_t i = 0; i < n_out; i++) { run.scores[i] = INT64_MIN; run.ids[i] = MSE_ID_NONE; }
    if (run.c->n != 0 && !(run.f && run.f->count == 0)) return 0;
    if (run.block_dev) {   // an empty shard still hands over a block: all slots empty
        if (launch_block_finish(nullptr, nullptr, n_out, 0, reinterpret_cast<int64_t*>(run.block_dev),
                                reinterpret_cast<uint32_t*>(static_cast<char*>(run.block_dev) + n_out * 8), nullptr)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return 1;
}

// all queries (+ scales) go up in ONE copy from pinned memory; every query then runs on the streams; ONE download at the end
int scan_upload(ScanRun& run, mse_searcher* s) {
    mse_pq* pq = run.pq;
    const size_t nq = run.nq, k = run.k, d = pq->d, lut_floats = pq->n_chunks * pq->n_centroids;
    const size_t sc_off = (nq * d * 4 + 255) & ~(size_t)255;
    const size_t sc_bytes = (run.scales && run.c->n_desc) ? run.c->n_desc * 4 : 0;
    const size_t in_bytes = sc_off + sc_bytes, out_bytes = nq * k * 12 + nq * 4;   // scores, ids, certificate flags
    run.prep_all = nq >= 4 && nq <= 2048;
    const size_t n_tab = run.prep_all ? nq : 8;
    if (pq->a.ensure(in_bytes + 256) || pq->b.ensure(n_tab * d * 4) || pq->c.ensure(n_tab * lut_floats * 4)) return -1;
    if (s->q_stage.ensure(8 * d * 2) || s->out_scores.ensure(out_bytes)) return -1;
    if (pq->pin.ensure(std::max(in_bytes, out_bytes), (size_t)1 << 16)) return -1;
    memcpy(pq->pin.p, run.queries_f32, nq * d * 4);
    if (sc_bytes) memcpy(pq->pin.as<char>() + sc_off, run.scales, sc_bytes);
    if (hipMemcpyAsync(pq->a.p, pq->pin.p, in_bytes, hipMemcpyHostToDevice, s->stream) != hipSuccess) return fail("H2D failed");
    run.queries_dev = pq->a.as<float>();
    run.scales_dev = sc_bytes ? reinterpret_cast<float*>(pq->a.as<char>() + sc_off) : nullptr;
    run.desc = run.scales_dev ? run.c->desc : nullptr;
    run.out_scores_dev = s->out_scores.as<int64_t>();
    run.out_ids_dev = reinterpret_cast<uint32_t*>(s->out_scores.as<char>() + nq * k * 8);
    run.flags_dev = reinterpret_cast<int*>(s->out_scores.as<char>() + nq * k * 12);
    run.lanes[0] = ScanLane{s, pq->b.as<float>(), pq->c.as<float>(), s->q_stage.as<uint16_t>()};
    return 0;
}

// Groups of queries alternate between TWO streams (each with its own scratch): the chain of small kernels that follows a scan
// (tournament, re-score of the nominated groups, selects, certificate) runs beside the next group's scan, on the CUs that scan leaves
// free.  (A third stream -- so that group u + 2 would not queue behind group u's tail -- and 16 / 24 / 32 spare CUs were measured in
// round 4: 0.194-0.203 ms per query at 32 per call in every combination, two streams and 8 spare CUs being the best; there is room
// for a third lane.)  Calls of fewer than four queries stay on the one lane.  A lane bound to another base than the call's is replaced.
int scan_lanes(ScanRun& run) {
    mse_pq* pq = run.pq;
    mse_searcher* s = run.lanes[0].s;
    const size_t d = pq->d;
    if (run.nq < 4) return 0;
    mse_searcher** extra[2] = {&pq->lane2, &pq->lane3};
    DevBuf* qfs[2] = {&pq->qf2, &pq->qf3};
#ifdef MSE_DEV_KERNELS
    static const int n_extra = getenv("MSE_PQ_LANES") ? std::min(std::max(atoi(getenv("MSE_PQ_LANES")) - 1, 0), 2) : 1;   // developer library: 1-3 streams
#else
    const int n_extra = 1;
#endif
    if (pq->t2.ensure(8 * d * 4) || pq->lut2.ensure(8 * pq->n_chunks * pq->n_centroids * 4)) return -1;
    for (int e = 0; e < n_extra; e++) {
        mse_searcher*& ln = *extra[e];
        if (ln && ln->base != s->base) { mse_searcher_free(ln); ln = nullptr; }
        if (!ln) ln = s->base ? mse_searcher_new(s->base) : scratch_searcher_new();
        if (!ln || qfs[e]->ensure(8 * d * 2)) return -1;
        run.lanes[e + 1] = ScanLane{ln, pq->t2.as<float>(), pq->lut2.as<float>(), qfs[e]->as<uint16_t>()};   // (several lanes imply prep_all)
        run.n_lanes = e + 2;
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess) return fail("H2D failed");   // uploads visible to every stream
    return 0;
}

// On the first lane's stream the flags' initial value and, for a prep_all call, every table; then the groups, alternating between the
// lanes; then every other lane has finished
int scan_dispatch(ScanRun& run) {
    mse_pq* pq = run.pq;
    hipStream_t st = run.lanes[0].s->stream;
    const size_t r = run.r;
    if (hipMemsetAsync(run.flags_dev, 0xff, run.nq * 4, st) != hipSuccess) return fail("memset failed");   // non-zero = certified / exact
    if (run.prep_all && (launch_pq_transform(pq->transform, (int)pq->d, run.queries_dev, run.nq, pq->b.as<float>(), st) ||
                         launch_pq_lut_batch(pq->centroids, (int)pq->n_centroids, (int)pq->d, (int)pq->dpc, pq->b.as<float>(), run.nq, pq->c.as<float>(), st)))
        return -1;
    if (run.n_lanes > 1 && hipStreamSynchronize(st) != hipSuccess) return fail("memset failed");
    run.four_ok = !run.list && pq_scan_gmax_supported((int)pq->n_chunks, (int)pq->n_centroids, run.desc, (int)run.c->n_desc, run.scales_dev) &&
                  r + std::max<size_t>(64, r / 2) + 1 <= (size_t)TOPK_KMAX;
    // eight per pass while the 8-bit certificate holds for this quantiser's data: a batch in which more than an eighth of the
    // eight-per-pass queries had to be repeated through the exact scan switches the handle back to four per pass for good
    run.eight_ok = run.four_ok && !pq->avoid8 && pq_nominated(r, 8) + 1 <= (size_t)TOPK_KMAX;
    bool ok = true;
    size_t q = 0;
    for (size_t unit = 0; q < run.nq && ok; unit++) {
        const ScanGroup g{(int)(unit % (size_t)run.n_lanes), q, scan_group_size(run.nq - q, run.eight_ok, run.four_ok, run.list)};
        ok = (g.n >= 4 ? scan_nominated_group(run, g) : scan_exact_group(run, g)) == 0;
        if (g.n == 8) run.n_in_eight += 8;   // (the eights come first: scan_group_size)
        q += g.n;
    }
    for (int w = 1; w < run.n_lanes; w++)
        if (hipStreamSynchronize(run.lanes[w].s->stream) != hipSuccess) ok = false;
    if (!ok) return std::string(mse_last_error()).empty() ? fail("scan failed") : -1;
    return 0;
}

// a query whose certificate did not hold (rare: the band of +-eps around its r-th score reached past the nominated groups) is
// repeated through the exact one-query scan, into the same output rows
int scan_repeat_uncertified(ScanRun& run) {
    mse_pq* pq = run.pq;
    hipStream_t st = run.lanes[0].s->stream;
    const size_t nq = run.nq;
    if (!run.four_ok || nq < 4) return 0;
    std::vector<int> flags(nq);
    if (hipMemcpyAsync(flags.data(), run.flags_dev, nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail("D2H failed");
    const size_t n8 = run.n_in_eight;
    size_t bad8 = 0;
    for (size_t j = 0; j < n8; j++) bad8 += !flags[j];
    // filtered batches are left out of this decision: a sparse filter legitimately fails more certificates (fewer than r allowed
    // vectors among the nominated groups), which says nothing about the quantiser's data
    if (!run.f && n8 && bad8 * 8 > n8) pq->avoid8 = true;
    for (size_t j = 0; j < nq; j++)
        if (!flags[j]) {
            pq->last_uncertified++;
            if (scan_exact_group(run, ScanGroup{0, j, 1})) return std::string(mse_last_error()).empty() ? fail("scan failed") : -1;
        }
    return 0;
}

// the results leave the first lane's stream: as a packed block on the device, or through the pinned staging into the caller's arrays
int scan_hand_over(const ScanRun& run) {
    mse_searcher* s = run.lanes[0].s;
    const size_t n_out = run.nq * run.k;
    if (run.block_dev) {
        if (launch_block_finish(run.out_scores_dev, run.out_ids_dev, n_out, run.id_offset, reinterpret_cast<int64_t*>(run.block_dev),
                                reinterpret_cast<uint32_t*>(static_cast<char*>(run.block_dev) + n_out * 8), s->stream) ||
            hipStreamSynchronize(s->stream) != hipSuccess) return fail("block hand-over failed");
        return 0;
    }
    if (hipMemcpyAsync(run.pq->pin.p, s->out_scores.p, n_out * 12, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess) return fail("D2H failed");
    memcpy(run.scores, run.pq->pin.p, n_out * 8);
    memcpy(run.ids, run.pq->pin.as<char>() + n_out * 8, n_out * 4);
    for (size_t i = 0; i < n_out; i++)
        if (run.ids[i] == MSE_ID_NONE) run.scores[i] = INT64_MIN;
    return 0;
}

// every lane is idle: the scan launches' event pairs can be read, and go back to the pools.  Two figures: each pair's own time
// (mse_pq_scan_timing), and the SUSTAINED rate -- from the first scan's start to the last scan's end of this call, over its scans (they
// run back to back, alternating between the streams: what a launch costs when the next one is already waiting behind it)
void scan_drain_timing(const ScanRun& run) {
    mse_pq* pq = run.pq;
    const mse_searcher* first = run.lanes[0].s;
    size_t scans = 0;
    float span = 0.0f;
    for (int w = 0; w < run.n_lanes; w++) {
        mse_searcher* ln = run.lanes[w].s;
        float ms = 0.0f;
        if (ln->ev_used >= 2 && first->ev_used >= 2) {
            if (hipEventElapsedTime(&ms, first->ev_pool[0], ln->ev_pool[ln->ev_used - 1]) == hipSuccess) span = std::max(span, ms);
            scans += ln->ev_used / 2;
        }
        for (size_t e = 0; e + 1 < ln->ev_used; e += 2)
            if (hipEventElapsedTime(&ms, ln->ev_pool[e], ln->ev_pool[e + 1]) == hipSuccess) { pq->scan_ms_total += ms; pq->scan_launches++; }
    }
    if (scans >= 4 && span > 0.0f) { pq->span_ms_total += span; pq->span_scans += scans; }
    for (int w = 0; w < run.n_lanes; w++) run.lanes[w].s->ev_used = 0;
}

// One call of the scan, for every entry point: all checks before anything is written; a call with nothing to do; the resolved mode of a
// filtered call (AUTO: the plan's answer for this call); then the steps.  s: the caller's searcher, or null for the quantiser's own.
// The unfiltered entry points make exactly the launches they always made.
int scan_call(ScanRun& run, mse_searcher* s) {
    if (check_pq_scan(run.pq, run.c, s, run.nq, run.r, run.k, run.fa)) return -1;
    if (run.nq == 0 || run.k == 0) return 0;
    if (!run.queries_f32 || !(run.block_dev || (run.scores && run.ids))) return fail("null argument");
    if (run.fa) {
        int mode = run.fa->mode;
        if (mode == MSE_PQ_FILTER_AUTO && mse_pq_filtered_plan(run.c->n, run.fa->f->count, run.nq, &mode)) return -1;
        run.f = run.fa->f;
        run.list = mode == MSE_PQ_FILTER_LIST;
        run.mask = run.f->words;
        run.mask_words = run.f->n_words;
    }
    mse_pq* pq = run.pq;
    run.r = std::max(run.r, run.k);
    if (const int rc = scan_answer_empty(run)) return rc < 0 ? -1 : 0;
    std::lock_guard<std::mutex> g(pq->mu);
    pq->last_uncertified = 0;
    if (!s) {
        if (!pq->scratch && !(pq->scratch = scratch_searcher_new())) return -1;
        s = pq->scratch;
    }
    if (scan_upload(run, s) || scan_lanes(run) || scan_dispatch(run) || scan_repeat_uncertified(run) || scan_hand_over(run))
        return -1;
    scan_drain_timing(run);
    return 0;
}

}  // namespace

extern "C" {

int mse_pq_scan_topk_batch(mse_pq* pq, const mse_codes* c, mse_searcher* s_or_null, const float* queries_f32, size_t nq,
                           const float* scales, size_t r, size_t k, int64_t* scores, uint32_t* ids) {
    if (!scores || !ids) return fail("null output");
    ScanRun run{pq, c, nullptr, nq, r, k, queries_f32, scales, nullptr, 0, scores, ids};
    return scan_call(run, s_or_null);
}

int mse_pq_scan_topk_block(mse_pq* pq, const mse_codes* c, mse_searcher* s_or_null, const float* queries_f32, size_t nq, const float* scales,
                           size_t r, size_t k, uint64_t id_offset, void* block_dev) {
    if (!block_dev) return fail("null output block");
    ScanRun run{pq, c, nullptr, nq, r, k, queries_f32, scales, block_dev, id_offset, nullptr, nullptr};
    return scan_call(run, s_or_null);
}

// test hook: the group maxima the flat scan nominates with -- lut1 == null: pq_scan64_kernel<true> for one table; otherwise
// pq_scan64x2_kernel for the pair.  out0 / out1: [ceil(n / 64)] i64 on the host.
static int debug_pq_group_max(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* lut0, const float* lut1, const float* scales,
                              int64_t* out0, int64_t* out1);
int mse_debug_pq_group_max(mse_pq* pq, const mse_codes* c, const float* lut0, const float* lut1, const float* scales, int64_t* out0,
                           int64_t* out1) {
    return debug_pq_group_max(pq, c, nullptr, lut0, lut1, scales, out0, out1);
}
// ... and the MASKED instantiations' maxima (INT64_MIN for a group without an allowed vector)
int mse_debug_pq_group_max_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* lut0, const float* lut1,
                                    const float* scales, int64_t* out0, int64_t* out1) {
    if (!pq || !c) return fail("null argument");
    if (check_pq_filter(pq, c, f)) return -1;
    return debug_pq_group_max(pq, c, f, lut0, lut1, scales, out0, out1);
}
static int debug_pq_group_max(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* lut0, const float* lut1, const float* scales,
                              int64_t* out0, int64_t* out1) {
    if (!pq || !c || !lut0 || !out0 || (lut1 && !out1)) return fail("null argument");
    if (c->code_size != pq->n_chunks) return fail("code size does not match the quantiser");
    const uint8_t* desc = (scales && c->n_desc) ? c->desc : nullptr;
    if (!pq_scan_gmax_supported((int)pq->n_chunks, (int)pq->n_centroids, desc, (int)c->n_desc, scales))
        return fail("the group-maximum scan serves 64 x 256 codecs (and 4 descriptor bytes) only");
    if (c->n == 0) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    const size_t lut_bytes = pq->n_chunks * pq->n_centroids * 4, n_groups = (c->n + 63) / 64;
    if (pq->a.ensure(2 * lut_bytes + 256) || pq->c.ensure(2 * n_groups * 8)) return -1;
    float* l0 = pq->a.as<float>();
    float* l1 = reinterpret_cast<float*>(pq->a.as<char>() + lut_bytes);
    float* sc = reinterpret_cast<float*>(pq->a.as<char>() + 2 * lut_bytes);
    MSE_HIP_TRY(hipMemcpy(l0, lut0, lut_bytes, hipMemcpyHostToDevice));
    if (lut1) MSE_HIP_TRY(hipMemcpy(l1, lut1, lut_bytes, hipMemcpyHostToDevice));
    if (desc) MSE_HIP_TRY(hipMemcpy(sc, scales, c->n_desc * 4, hipMemcpyHostToDevice));
    int64_t* g0 = pq->c.as<int64_t>();
    int64_t* g1 = g0 + n_groups;
    const uint32_t* mw = f ? f->words : nullptr;
    const size_t mn = f ? f->n_words : 0;
    const int rc = lut1 ? launch_pq_scan_gmax2(l0, l1, c->codes, c->n, desc, desc ? sc : nullptr, g0, g1, device_cu_count(), nullptr, mw, mn)
                        : launch_pq_scan_gmax(l0, c->codes, c->n, desc, desc ? sc : nullptr, g0, device_cu_count(), nullptr, mw, mn);
    if (rc) return -1;
    MSE_HIP_TRY(hipMemcpy(out0, g0, n_groups * 8, hipMemcpyDeviceToHost));
    if (lut1) MSE_HIP_TRY(hipMemcpy(out1, g1, n_groups * 8, hipMemcpyDeviceToHost));
    return 0;
}

// HIP-event timing of the four-queries-per-pass scan kernel (the dominant kernel of a batched scan): returns the totals so far,
// then sets the mode: 0 off, 1 on, 2 on and reset
int mse_pq_scan_timing(mse_pq* pq, int enable, double* total_ms, uint64_t* launches) {
    if (!pq) return fail("null quantiser");
    std::lock_guard<std::mutex> g(pq->mu);
    if (total_ms) *total_ms = pq->scan_ms_total;
    if (launches) *launches = pq->scan_launches;
    if (enable == 2) { pq->scan_ms_total = 0.0; pq->scan_launches = 0; pq->span_ms_total = 0.0; pq->span_scans = 0; }
    pq->timing = enable != 0;
    return 0;
}

// The SUSTAINED figure beside it: over the batch calls made while timing was on that ran at least four scans, the time from the first
// scan's start to the last scan's end (HIP events) and the number of scans in those spans.  span / scans = what a pass costs when passes
// run back to back (two streams, a group's tail beside the next group's scan); reset by mse_pq_scan_timing(pq, 2, ..).
int mse_pq_scan_sustained(mse_pq* pq, double* span_ms, uint64_t* scans) {
    if (!pq) return fail("null quantiser");
    std::lock_guard<std::mutex> g(pq->mu);
    if (span_ms) *span_ms = pq->span_ms_total;
    if (scans) *scans = pq->span_scans;
    return 0;
}

// PQ codes of rows that are already resident in HBM: quantize_batch (vector.rs:331-364) over f32 widenings of the base's f16 rows
// (what dump_processor feeds it, src/dump_processor.rs:468-481), 65536 rows at a time on the device; only the descriptors cross
// PCIe.  The codes equal mse_pq_quantize_batch's on the same rows.
mse_codes* mse_codes_quantize_base(mse_pq* pq, const mse_base* b, const uint8_t* descriptors, size_t n_descriptors) {
    if (!pq || !b) { fail("null quantiser or base"); return nullptr; }
    if (b->d != pq->d) { fail("base width differs from the quantiser"); return nullptr; }
    mse_codes* c = new (std::nothrow) mse_codes();
    if (!c) { fail("out of host memory"); return nullptr; }
    const size_t n = b->n, cs = pq->n_chunks;
    c->n = n; c->code_size = cs; c->n_desc = descriptors ? n_descriptors : 0;
    bool ok = hipMalloc((void**)&c->codes, n * cs + 4096) == hipSuccess;
    if (ok && c->n_desc) {
        ok = hipMalloc((void**)&c->desc, n * c->n_desc + 256) == hipSuccess;
        if (ok && n) ok = hipMemcpy(c->desc, descriptors, n * c->n_desc, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        std::lock_guard<std::mutex> g(pq->mu);
        const size_t step = 65536;
        ok = pq->a.ensure(step * pq->d * 4) == 0 && pq->b.ensure(step * pq->d * 4) == 0;
        for (size_t r0 = 0; ok && r0 < n; r0 += step) {
            const size_t m = std::min(step, n - r0);
            ok = launch_f16_to_f32(b->dev + r0 * b->d, m * b->d, pq->a.as<float>(), nullptr) == 0 &&
                 launch_pq_transform(pq->transform, (int)pq->d, pq->a.as<float>(), m, pq->b.as<float>(), nullptr) == 0 &&
                 launch_pq_quantize(pq->centroids, (int)pq->n_centroids, (int)pq->d, (int)pq->dpc, pq->b.as<float>(), m, c->codes + r0 * cs, nullptr) == 0;
        }
        if (ok) ok = hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) { mse_codes_free(c); if (std::string(mse_last_error()).empty()) fail("device allocation / quantisation failed"); return nullptr; }
    return c;
}

// test hook: the integer nomination scan by itself -- the four queries' group maxima (u32, [4][ceil(n / 64)]) and their
// certificate parameters (params_out [4][4] = delta, c, eps, ok), so that a test can rebuild the 12-bit tables on the host and
// check every maximum of the matrix-core scan against plain integer sums
static int debug_pq4_group_max(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* luts4, const float* scales, int n_valid,
                               int per_pass, uint32_t* out, double* params_out);
int mse_debug_pq4_group_max(mse_pq* pq, const mse_codes* c, const float* luts4, const float* scales, int n_valid, int per_pass, uint32_t* out,
                            double* params_out) {
    return debug_pq4_group_max(pq, c, nullptr, luts4, scales, n_valid, per_pass, out, params_out);
}
// ... and the MASKED instantiations' maxima (the zero-sum key 0 for a group without an allowed vector)
int mse_debug_pq4_group_max_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* luts4, const float* scales, int n_valid,
                                     int per_pass, uint32_t* out, double* params_out) {
    if (!pq || !c) return fail("null argument");
    if (check_pq_filter(pq, c, f)) return -1;
    return debug_pq4_group_max(pq, c, f, luts4, scales, n_valid, per_pass, out, params_out);
}
static int debug_pq4_group_max(mse_pq* pq, const mse_codes* c, const mse_filter* f, const float* luts4, const float* scales, int n_valid,
                               int per_pass, uint32_t* out, double* params_out) {
    if (!pq || !c || !luts4 || !out || !params_out) return fail("null argument");
    if (per_pass != 4 && per_pass != 8) return fail("per_pass must be 4 or 8");
    const size_t NQ = (size_t)per_pass;
    if (c->code_size != pq->n_chunks || pq->n_chunks != 64 || pq->n_centroids != 256) return fail("the four-query scan serves 64 x 256 codecs only");
    if (n_valid < 1 || n_valid > per_pass) return fail("n_valid must be 1 .. per_pass");
    const uint8_t* desc = (scales && c->n_desc) ? c->desc : nullptr;
    if (desc && c->n_desc != 4) return fail("the four-query scan takes 4 descriptor bytes");
    if (c->n == 0) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    const size_t lut_bytes = NQ * 64 * 256 * 4, n_groups = (c->n + 63) / 64;
    if (pq->a.ensure(lut_bytes + 256) || pq->b.ensure(pq4_table_bytes() + 8 * sizeof(Pq4Params)) || pq->c.ensure(NQ * n_groups * 4)) return -1;
    float* sc = reinterpret_cast<float*>(pq->a.as<char>() + lut_bytes);
    MSE_HIP_TRY(hipMemcpy(pq->a.p, luts4, lut_bytes, hipMemcpyHostToDevice));
    if (desc) MSE_HIP_TRY(hipMemcpy(sc, scales, 16, hipMemcpyHostToDevice));
    Pq4Params* params = reinterpret_cast<Pq4Params*>(pq->b.as<char>() + pq4_table_bytes());
    if (launch_pq4_table(pq->a.as<float>(), desc ? sc : nullptr, n_valid, pq->b.p, params, nullptr, per_pass)) return -1;
    if (launch_pq_scan_gmax4(pq->b.p, c->codes, c->n, desc, pq->c.as<uint32_t>(), device_cu_count(), nullptr, per_pass, f ? f->words : nullptr,
                             f ? f->n_words : 0)) return -1;
    Pq4Params ph[8];
    {   // the scan writes group-major [n_groups][NQ]; the hook hands out [NQ][n_groups]
        std::vector<uint32_t> gm(NQ * n_groups);
        MSE_HIP_TRY(hipMemcpy(gm.data(), pq->c.p, NQ * n_groups * 4, hipMemcpyDeviceToHost));
        for (size_t g2 = 0; g2 < n_groups; g2++)
            for (size_t j = 0; j < NQ; j++) out[j * n_groups + g2] = gm[g2 * NQ + j];
    }
    MSE_HIP_TRY(hipMemcpy(ph, params, NQ * sizeof(Pq4Params), hipMemcpyDeviceToHost));
    for (int j = 0; j < per_pass; j++) { params_out[4 * j] = ph[j].delta; params_out[4 * j + 1] = ph[j].c; params_out[4 * j + 2] = ph[j].eps; params_out[4 * j + 3] = ph[j].ok; }
    return 0;
}

// queries of the last mse_pq_scan_topk_batch call whose four-query certificate did not hold and that were repeated through the
// exact scan (0 for batches of fewer than four queries)
uint32_t mse_pq_last_uncertified(mse_pq* pq) {
    if (!pq) return 0;
    std::lock_guard<std::mutex> g(pq->mu);
    return pq->last_uncertified;
}

// One query per call, possibly from many threads at once (the reference: one greedy_search / evaluate per request on a thread per
// core, src/query_disk_index.rs:711-736).  Calls meet in the quantiser's coalescer; the worker sorts what it gathered into groups
// that can share a batch call -- same codes, same base rows (or none), same r and k, the same descriptor scales byte for byte --
// and runs each group through mse_pq_scan_topk_batch (four queries per pass over the codes), on the searcher of the group's first
// caller (its owner is blocked in this call, so it is free to borrow).  Results are those of the call made alone.
namespace {
struct PqKey {
    const mse_codes* c; const mse_base* base; size_t r, k; const float* scales; size_t n_sc;
    bool same(const PqKey& o) const {
        if (c != o.c || base != o.base || r != o.r || k != o.k || (scales == nullptr) != (o.scales == nullptr)) return false;
        return !scales || (n_sc == o.n_sc && memcmp(scales, o.scales, n_sc * 4) == 0);
    }
};
PqKey pq_key_of(const DispatchReq* q) {
    const mse_codes* c = static_cast<const mse_codes*>(q->aux0);
    const mse_searcher* s = static_cast<const mse_searcher*>(q->aux1);
    return PqKey{c, s ? s->base : nullptr, q->aux_n, q->k, static_cast<const float*>(q->aux2), c->n_desc};
}
void pq_run_batch(mse_pq* pq, std::vector<DispatchReq*>& batch) {
    std::vector<float> qs;
    std::vector<int64_t> sc;
    std::vector<uint32_t> id;
    // one batch call for requests of the same key, on the searcher of the first (alone: the caller's own searcher)
    auto run_group = [&](std::vector<DispatchReq*>& grp) {
        const PqKey key = pq_key_of(grp[0]);
        const size_t d = pq->d, k = key.k;
        run_shared(grp, [&](DispatchReq* const* reqs, size_t n) {
            qs.resize(n * d); sc.resize(n * k); id.resize(n * k);
            for (size_t j = 0; j < n; j++) memcpy(qs.data() + j * d, reqs[j]->queries, d * 4);
            mse_searcher* s = const_cast<mse_searcher*>(static_cast<const mse_searcher*>(reqs[0]->aux1));
            const int rc = mse_pq_scan_topk_batch(pq, key.c, s, qs.data(), n, key.scales, key.r, k, sc.data(), id.data());
            for (size_t j = 0; rc == 0 && j < n; j++) {
                memcpy(reqs[j]->out_a, sc.data() + j * k, k * 8);
                memcpy(reqs[j]->out_b, id.data() + j * k, k * 4);
            }
            return rc;
        });
    };
    for_each_shared_group(batch, [](const DispatchReq& a, const DispatchReq& b) { return pq_key_of(&a).same(pq_key_of(&b)); }, run_group);
}
}  // namespace

int mse_pq_scan_topk(mse_pq* pq, const mse_codes* c, mse_searcher* s_or_null, const float* query_f32,
                     const float* scales, size_t r, size_t k, int64_t* scores, uint32_t* ids) {
    // argument errors belong to this caller alone: they never enter the queue
    if (check_pq_scan(pq, c, s_or_null, 1, r, k, nullptr)) return -1;
    if (!query_f32 || !scores || !ids) return fail("null argument");
    if (k == 0) return 0;
    {
        std::lock_guard<std::mutex> g(pq->co_mu);
        if (!pq->co) {
            const int device = pq->device;
            // up to 64 queries per gather (sixteen passes of four); wait budget from the size of the first code array seen
            pq->co = new (std::nothrow) Coalescer(64, default_wait_us(c->n, c->code_size + c->n_desc),
                                                  [pq](std::vector<DispatchReq*>& b) { pq_run_batch(pq, b); },
                                                  [device] { (void)hipSetDevice(device); });
            if (!pq->co) return fail("out of host memory");
        }
    }
    DispatchReq q;
    q.queries = query_f32; q.nq = 1; q.k = k; q.out_a = scores; q.out_b = ids;
    q.aux0 = c; q.aux1 = s_or_null; q.aux2 = (scales && c->n_desc) ? scales : nullptr; q.aux_n = r;
    return pq->co->submit(q);
}

// ---- the flat scan over an allowed-row set (include/mse.h) ----
// Where LIST overtakes SCAN.  The rule is a count of bytes:
//   SCAN streams 64 code bytes + 4 descriptor bytes for every one of the n rows, once per PASS; a batch of nq queries makes
//        nq / 8 passes of eight, then one of four, one pair and one single for what is left (scan_group_size);
//   LIST gathers one 64-byte code row + 4 descriptor bytes per allowed row PER QUERY.  A gathered 64-byte row occupies half of a
//        128-byte line, so unless its neighbour is allowed too it moves twice its size: PQ_LIST_BYTE_COST = 2.
// That alone -- LIST when nq * allowed * 2 <= passes * n -- was the first, unmeasured form.  Measured once (scripts/filtered_pq_probe.py,
// profiles/filtered_pq_probe.json: one MI355X, 1e7 codes, r 200) the curves cross at allowed / n = 0.42 for one query (the rule: 0.5,
// i.e. a byte cost of 2.4 against the assumed 2: kept), but at 0.020 for eight and 0.0022 for thirty-two queries where the rule said
// 0.0625 for both: a LIST query is a chain of small launches (gather, tournament, map, re-score) that costs ~0.04 ms whatever the
// list's length and does not overlap its neighbours the way the tails of batched scans do.  So a FIXED cost per LIST query was added,
// in streamed-byte equivalents: PQ_LIST_FIXED_BYTES = 1.2e6 rows x 68 B.  With it the rule gives 0.44 / 0.0025 / 0.0025 at the three
// batch sizes: right for 1 and 32, cautious for 8 (between 0.0025 and 0.02 it keeps the masked scan, which is at most 12 % slower
// there).  One box, one size: both constants stay PROVISIONAL; at 1e8 codes the fixed term matters a tenth as much.
// Monotone in `allowed` by construction; an index below 1.2e6 rows always scans (unless nothing is allowed).
static constexpr double PQ_ROW_BYTES = 68.0, PQ_LIST_BYTE_COST = 2.0, PQ_LIST_FIXED_BYTES = 1.2e6 * 68.0;
int mse_pq_filtered_plan(size_t n_codes, size_t allowed, size_t nq, int* mode_out) {
    if (!mode_out) return fail("pq_filtered_plan: null argument");
    if (allowed > n_codes) return fail("pq_filtered_plan: more allowed rows than codes");
    if (nq == 0) return fail("pq_filtered_plan: nq must be positive");
    size_t passes = nq / 8;   // the eights, then the groups the dispatch makes of what is left
    for (size_t rem = nq % 8; rem; rem -= (size_t)scan_group_size(rem, true, true, false)) passes++;
    // (in double: the products pass 2^64 only far beyond any real call, but the comparison must not wrap)
    const double list_cost = (double)nq * ((double)allowed * PQ_ROW_BYTES * PQ_LIST_BYTE_COST + PQ_LIST_FIXED_BYTES);
    const double scan_cost = (double)passes * (double)n_codes * PQ_ROW_BYTES;
    *mode_out = (allowed == 0 || list_cost <= scan_cost) ? MSE_PQ_FILTER_LIST : MSE_PQ_FILTER_SCAN;
    return 0;
}

int mse_pq_scan_topk_batch_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, mse_searcher* s_or_null, const float* queries_f32,
                                    size_t nq, const float* scales, size_t r, size_t k, int mode, int64_t* scores, uint32_t* ids) {
    const PqFilterArg fa{f, mode};
    ScanRun run{pq, c, &fa, nq, r, k, queries_f32, scales, nullptr, 0, scores, ids};
    return scan_call(run, s_or_null);
}
// (one query per call: straight to the batch path -- filtered calls do not meet in the quantiser's coalescer)
int mse_pq_scan_topk_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, mse_searcher* s_or_null, const float* query_f32,
                              const float* scales, size_t r, size_t k, int mode, int64_t* scores, uint32_t* ids) {
    return mse_pq_scan_topk_batch_filtered(pq, c, f, s_or_null, query_f32, 1, scales, r, k, mode, scores, ids);
}
int mse_pq_scan_topk_block_filtered(mse_pq* pq, const mse_codes* c, const mse_filter* f, mse_searcher* s_or_null, const float* queries_f32,
                                    size_t nq, const float* scales, size_t r, size_t k, int mode, uint64_t id_offset, void* block_dev) {
    const PqFilterArg fa{f, mode};
    ScanRun run{pq, c, &fa, nq, r, k, queries_f32, scales, block_dev, id_offset, nullptr, nullptr};
    return scan_call(run, s_or_null);
}

int64_t mse_descriptor_product(const float* scales, size_t n_descriptors, const uint8_t* descriptors, uint32_t id) {
    // src/query_disk_index.rs:135-142 (host helper; the device paths fold the same sum into their kernels)
    int64_t r = 0;
    for (size_t j = 0; j < n_descriptors; j++)
        r += scale_dot_result(scales[j] * (float)descriptors[(size_t)id * n_descriptors + j]);
    return r;
}

}  // extern "C"
