// C ABI (include/mse.h): the brute-force search -- the exact-order pass, the matrix-core pass with its certificate, and the entry points
// of both, filtered and unfiltered.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>

namespace mse {

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

// The pass itself: rows ids[0 .. n) (ascending; null = rows 0 .. n), and -- the filtered graph search's LIST regime -- the descriptor
// bias of every listed row added to its score BEFORE the selection (bias: descriptors, their count, the pass's scales on the device).
// With a grouping g (nq_pass <= dense_pass_queries(g->n_rows, 12)) it is the grouped search's dense pass: the scan leaves every eligible
// row's score in level 0; the group step (group.hip) finds each group's best row and drops every other grouped row to INT64_MIN; the
// tournament then ranks representatives before everything it has to, and the collapse of its k results removes the demoted rows that
// filled a short list -- each comes after its own representative, which has the higher score or the lower id.  Level 0 holds list
// positions when ids are given: the group step maps them through the list.  Representatives whose own score saturates to INT64_MIN tie
// with the demoted rows and can be crowded off the list: a short list is completed from them afterwards (group.hip
// dense_complete_kernel).  Grouped results go to row dst_rows[j] (device; null: j) of the outputs.
int exact_pass_list(mse_searcher* s, int nq_pass, int k, uint64_t id_offset, int64_t* out_scores, uint32_t* out_ids, size_t out_stride,
                    const uint32_t* ids, size_t n, const ListBias* bias, const mse_groups* g, const uint32_t* dst_rows) {
    const mse_base* b = s->base;
    hipStream_t st = s->stream;
    if (s->scores.ensure((size_t)nq_pass * n * 8)) return -1;
    const bool tm = g && s->grp_timing;
    if (tm) MSE_HIP_TRY(hipEventRecord(s->grp_ev[0], st));
    if (launch_scan_exact(b->dev, n, (int)b->d, s->q_stage.p, nq_pass, false, s->scores.as<int64_t>(), n, nullptr,
                          s->n_cu, st, ids)) return -1;
    if (bias && launch_list_bias(ids, n, bias->desc, bias->n_desc, bias->scales_dev, nq_pass, s->scores.as<int64_t>(), n, st)) return -1;
    if (tm) MSE_HIP_TRY(hipEventRecord(s->grp_ev[1], st));
    unsigned long long* best = nullptr;
    uint32_t *best_id = nullptr, *n_sat = nullptr;
    if (g && g->n_rows) {   // group table: best keys [nq][g_len] u64 | best ids [nq][g_len] u32 | saturated representatives [nq] u32
        if (s->grp_best.ensure((size_t)nq_pass * g->n_rows * 12 + (size_t)nq_pass * 4)) return -1;
        best = s->grp_best.as<unsigned long long>();
        best_id = reinterpret_cast<uint32_t*>(best + (size_t)nq_pass * g->n_rows);
        n_sat = best_id + (size_t)nq_pass * g->n_rows;
        if (launch_dense_group_best(false, s->scores.p, n, n, ids, g->group_of, g->n_rows, nq_pass, best, best_id, n_sat, st)) return -1;
    }
    if (tm) MSE_HIP_TRY(hipEventRecord(s->grp_ev[2], st));
    if (s->sel_keys.ensure((size_t)nq_pass * k * 8)) return -1;
    uint32_t* sel = nullptr;
    LevelRef l0{KEY_I64, s->scores.p, n, 1, n, false, 0};
    if (descend(s, l0, nq_pass, k, &sel, s->sel_keys.p)) return -1;
    if (ids && launch_map_positions(sel, (size_t)nq_pass * k, ids, st)) return -1;
    if (!g)
        return launch_finalize(sel, s->sel_keys.as<int64_t>(), k, k, nq_pass, id_offset, out_scores, out_ids, out_stride,
                               nullptr, 0, 0, 0, nullptr, nullptr, st);
    if (s->grp_pos.ensure((size_t)nq_pass * k * 4) || s->grp_reps.ensure((size_t)nq_pass * 4)) return -1;
    uint32_t *kept = s->grp_pos.as<uint32_t>(), *reps = s->grp_reps.as<uint32_t>();
    if (launch_collapse(sel, (size_t)k, (size_t)k, g->group_of, g->n_rows, k, nq_pass, kept, reps, st)) return -1;
    if (launch_collapse_gather(kept, k, sel, (size_t)k, s->sel_keys.p, (size_t)k, 8, nq_pass, id_offset, dst_rows, nullptr, out_scores, out_ids,
                               out_stride, st)) return -1;
    if (launch_dense_complete(s->scores.as<int64_t>(), n, n, ids, g->group_of, g->n_rows, best_id, n_sat, kept, reps, s->sel_keys.as<int64_t>(), k,
                              nq_pass, id_offset, dst_rows, out_scores, out_ids, out_stride, st)) return -1;
    if (tm) {
        MSE_HIP_TRY(hipEventRecord(s->grp_ev[3], st));
        MSE_HIP_TRY(hipEventSynchronize(s->grp_ev[3]));
        for (int i = 0; i < 3; i++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, s->grp_ev[i], s->grp_ev[i + 1]) == hipSuccess) s->grp_ms[i + 1] += ms;
        }
    }
    return 0;
}

// exact mode, one pass of <= 8 queries: rows pick[0 .. nq_pass) of q_dev (null: its first nq_pass rows) are staged, zero-padded to 8, in
// s->q_stage.  With a filter (non-empty, no longer than the base): the filter's allowed rows only, scanned through its ascending id list;
// level 0 then holds list positions, so an excluded row is absent -- not merely low: an allowed row whose score saturates to INT64_MIN
// still ranks -- and (score desc, position asc) is (score desc, id asc).  The selected positions are mapped back to row ids before the finish.
static int stage_exact_queries(mse_searcher* s, const uint16_t* q_dev, const uint32_t* pick, int nq_pass) {
    const size_t row = s->base->d * 2;
    if (s->q_stage.ensure(8 * row)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(s->q_stage.p, 0, 8 * row, s->stream));
    if (!pick) MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.p, q_dev, nq_pass * row, hipMemcpyDeviceToDevice, s->stream));
    for (int j = 0; pick && j < nq_pass; j++)
        MSE_HIP_TRY(hipMemcpyAsync(s->q_stage.as<char>() + j * row, reinterpret_cast<const char*>(q_dev) + pick[j] * row, row,
                                   hipMemcpyDeviceToDevice, s->stream));
    return 0;
}

static int exact_pass(mse_searcher* s, const mse_filter* f, const uint16_t* q_dev, const uint32_t* pick, int nq_pass, int k, uint64_t id_offset,
                      int64_t* out_scores, uint32_t* out_ids, size_t out_stride) {
    if (stage_exact_queries(s, q_dev, pick, nq_pass)) return -1;
    return exact_pass_list(s, nq_pass, k, id_offset, out_scores, out_ids, out_stride, f ? f->ids : nullptr, f ? f->count : s->base->n, nullptr);
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
// the re-score and the widening only ever touch the nq real rows.
// The stages, in the order the pass runs them: the scan (scan_dense or scan_sparse) leaves the group maxima of every query behind as a
// GroupMaxima; certified_round picks a query's best groups from one and certifies its answer; first_round runs one over all queries and
// sorts out who is done; widen carries the others on as a compact set, round by round; exact_rest is for whom no round can certify.
struct Pass {
    mse_searcher* s; const mse_base* b; hipStream_t st;   // the searcher, its base, its stream
    const mse_filter* f;                                  // null: every row
    const uint16_t* q; int nq, k;                         // [nq][d] f16 on the device, 16-byte aligned
    uint64_t id_offset; int64_t* out_scores; uint32_t* out_ids; size_t out_stride;
    int d, tile, n_full, rem, nq_pad;   // n_full passes of `tile` queries and one of rem, padded: nq_pad columns
    int gr; size_t n_groups;            // rows per group maximum, and how many groups that makes
    int kg0;                            // groups the first round re-scores per query
};

// the sparse form's lists, carved from one buffer: thresholds [nq] f32 | survivor counts [nq] u32 | group ids [nq][cap] u32 | maxima [nq][cap] f32
struct ListSrc { uint32_t* ids; float* keys; uint32_t* counts; float* tau; };
static ListSrc carve_lists(const DevBuf& buf, size_t nq, uint32_t cap) {
    float* tau = buf.as<float>();
    uint32_t* counts = reinterpret_cast<uint32_t*>(tau + nq);
    return ListSrc{counts + nq, reinterpret_cast<float*>(counts + nq + nq * cap), counts, tau};
}

// What a scan leaves behind, in one of two forms.  Dense: the array of group maxima [n_groups][pad].  Sparse (scan_sparse): per query
// the list of the groups whose maximum is above its threshold, `cap` entries at most; counts_h: where the counts -- how many groups
// WANTED onto each list -- reach the host with the next round's synchronisation.
struct GroupMaxima {
    bool sparse;
    const float* dense; int pad;
    ListSrc lists; uint32_t cap; const uint32_t* counts_h;
};

// Thresholded group maxima (the 320-query unmasked pass with 64-row groups only).  The dense array of group
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

// |mfma score - exact-order score| <= 2 * gamma_1151 * sum|x_i q_i| <= 1.4e-4 * |x||q|; doubled again
// because the matrix core's internal rounding is not documented.
static int query_eps(const Pass& p, const uint16_t* q, int nq, float* eps) {
    return launch_query_eps(q, nq, p.d, p.b->norm_bits_dev, 2.8e-4f, eps, p.st);
}

// Stage 1, dense: the full passes go out as ONE launch (a small base has few row tiles: its passes fill the chip side by side), then the
// remainder; their columns lie side by side in the array of group maxima.
static int scan_dense(const Pass& p, GroupMaxima* gm) {
    mse_searcher* s = p.s;
    if (s->gmax.ensure(p.n_groups * (size_t)p.nq_pad * 4)) return -1;
    const uint32_t* mask = p.f ? p.f->words : nullptr;
    const size_t mask_words = p.f ? p.f->n_words : 0;
    const int done = p.n_full * p.tile;   // queries the full passes take
    if (p.n_full &&
        launch_scan_mfma(p.b->dev, p.b->n, p.d, p.q, p.tile, s->qpacked.p, s->gmax.as<float>(), s->n_cu, p.st,
                         s->timing ? s->ev0 : nullptr, s->timing && !p.rem ? s->ev1 : nullptr, p.nq_pad, p.n_full, mask, mask_words, done, p.gr)) return -1;
    if (p.rem &&
        launch_scan_mfma(p.b->dev, p.b->n, p.d, p.q + (size_t)done * p.d, p.nq_pad - done, s->qpacked.p,
                         s->gmax.as<float>() + done, s->n_cu, p.st, s->timing && !p.n_full ? s->ev0 : nullptr,
                         s->timing ? s->ev1 : nullptr, p.nq_pad, 1, mask, mask_words, p.rem, p.gr)) return -1;
    if (query_eps(p, p.q, p.nq, s->eps.as<float>())) return -1;
    *gm = GroupMaxima{false, s->gmax.as<float>(), p.nq_pad, ListSrc{}, 0, nullptr};
    return 0;
}

// Stage 1, sparse (SparsePlan above): the sample, the thresholds from it (which need eps already), the other tiles onto the lists.
static int scan_sparse(const Pass& p, const SparsePlan& sp, GroupMaxima* gm) {
    mse_searcher* s = p.s;
    const uint32_t cap = sp.cap;
    if (s->sp_dense.ensure(sp.n_a * 4 * (size_t)320 * 4) || s->sp_lists.ensure((size_t)320 * 8 + (size_t)320 * cap * 8) ||
        s->sp_pin.ensure((size_t)320 * 4, 4096)) return -1;
    const ListSrc L = carve_lists(s->sp_lists, 320, cap);
    ScanSparse a;
    a.n_tiles = sp.n_a; a.mul = sp.stride; a.shift = 63; a.add = 0;
    if (launch_scan_mfma_tiles(p.b->dev, p.b->n, p.d, p.q, p.nq, true, s->qpacked.p, a, s->sp_dense.as<float>(), s->n_cu, p.st,
                               s->timing ? s->ev0 : nullptr, nullptr)) return -1;
    if (query_eps(p, p.q, p.nq, s->eps.as<float>())) return -1;
    if (s->gkeys.ensure((size_t)p.nq * p.k * 4)) return -1;
    uint32_t* ssel = nullptr;
    LevelRef ls0{KEY_F32, s->sp_dense.p, 1, (size_t)320, sp.n_sg, true, 320};
    if (descend(s, ls0, p.nq, p.k, &ssel, s->gkeys.p)) return -1;
    if (launch_sparse_tau(s->gkeys.as<float>(), (size_t)p.k, p.k, s->eps.as<float>(), p.nq, 320, L.tau, L.counts, p.st)) return -1;
    if (launch_sparse_append_sample(s->sp_dense.as<float>(), 320, sp.n_sg, p.nq, sp.stride, L.tau, L.counts, L.ids, L.keys, cap, p.st)) return -1;
    ScanSparse bb;
    bb.n_tiles = sp.n_b; bb.mul = 1; bb.shift = sp.shift; bb.add = 1;   // the j-th tile that is no multiple of S: j + j / (S - 1) + 1
    bb.tau = L.tau; bb.counts = L.counts; bb.ids = L.ids; bb.keys = L.keys; bb.cap = cap;
    if (launch_scan_mfma_tiles(p.b->dev, p.b->n, p.d, p.q, p.nq, false, s->qpacked.p, bb, nullptr, s->n_cu, p.st, nullptr,
                               s->timing ? s->ev1 : nullptr)) return -1;
    // the counts reach the host with the first round's margins (its synchronisation)
    MSE_HIP_TRY(hipMemcpyAsync(s->sp_pin.p, L.counts, (size_t)320 * 4, hipMemcpyDeviceToHost, p.st));
    *gm = GroupMaxima{true, nullptr, 0, L, cap, s->sp_pin.as<uint32_t>()};
    return 0;
}

// Stage 2.  One round of: the kg best groups of each query from gm (dense: a tournament over the group maxima; sparse: a selection from
// the query's list) -> their rows re-scored exactly -> exact top-k -> certificate.  gm holds the maxima of the nq queries in `qs`
// ([nq][d] f16); results go to dst_* with stride dst_stride; the margins (> 0 = certified) come back into pinned memory --
// s->margin_pin [0 .. nq) -- by a true asynchronous copy, then the one synchronisation that ends the round.
static int certified_round(const Pass& p, const GroupMaxima& gm, const uint16_t* qs, int nq, int kg, const float* eps_dev, float* margin_dev,
                           int64_t* dst_s, uint32_t* dst_i, size_t dst_stride) {
    mse_searcher* s = p.s;
    const mse_filter* f = p.f;
    const int k = p.k;
    if (s->gkeys.ensure((size_t)nq * kg * 4)) return -1;
    uint32_t* gsel = nullptr;
    const float* tau = nullptr;   // the sparse form: what is not on a list is at most the query's threshold
    if (gm.sparse) {
        if (s->sel_a.ensure((size_t)nq * kg * 4)) return -1;
        gsel = s->sel_a.as<uint32_t>();
        tau = gm.lists.tau;
        SelectArgs a{};
        a.kind = KEY_F32; a.list_ids = gm.lists.ids; a.list_keys = gm.lists.keys; a.list_stride = gm.cap; a.n_list = gm.cap; a.list_count = gm.lists.counts;
        a.k = kg; a.out_ids = gsel; a.out_keys = s->gkeys.p; a.out_stride = kg; a.nq = nq;
        if (launch_select(a, p.st)) return -1;
    } else {
        LevelRef l0{KEY_F32, gm.dense, 1, (size_t)gm.pad, p.n_groups, true, gm.pad};
        if (descend(s, l0, nq, kg, &gsel, s->gkeys.p)) return -1;
    }
    const size_t n_cand = (size_t)kg * p.gr;
    if (s->cand_ids.ensure((size_t)nq * n_cand * 4) || s->cand_scores.ensure((size_t)nq * n_cand * 8)) return -1;
    if (f ? launch_expand_groups_masked(gsel, kg, kg, p.gr, p.b->n, f->words, f->n_words, s->cand_ids.as<uint32_t>(), n_cand, nq, p.st)
          : launch_expand_groups(gsel, kg, kg, p.gr, p.b->n, s->cand_ids.as<uint32_t>(), n_cand, nq, p.st)) return -1;
    if (launch_score_rows(p.b->dev, p.b->n, p.d, qs, false, s->cand_ids.as<uint32_t>(), (size_t)nq * n_cand, n_cand,
                          s->cand_scores.as<int64_t>(), nullptr, p.st)) return -1;
    // final exact selection among the re-scored candidates
    if (s->sel_keys.ensure((size_t)nq * k * 8) || s->misc.ensure((size_t)nq * k * 4)) return -1;
    SelectArgs a{};
    a.kind = KEY_I64; a.list_ids = s->cand_ids.as<uint32_t>(); a.list_keys = s->cand_scores.p;
    a.list_stride = n_cand; a.n_list = n_cand; a.k = k; a.out_ids = s->misc.as<uint32_t>();
    a.out_keys = s->sel_keys.p; a.out_stride = k; a.nq = nq;
    if (launch_select(a, p.st)) return -1;
    if (launch_finalize(s->misc.as<uint32_t>(), s->sel_keys.as<int64_t>(), k, k, nq, p.id_offset, dst_s, dst_i, dst_stride,
                        s->gkeys.as<float>(), kg, kg, p.n_groups, eps_dev, margin_dev, p.st, tau)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(s->margin_pin.p, margin_dev, (size_t)nq * 4, hipMemcpyDeviceToHost, p.st));
    MSE_HIP_TRY(hipStreamSynchronize(p.st));
    s->last_max_groups = std::max<uint32_t>(s->last_max_groups, (uint32_t)kg);
    return 0;
}

// Stage 5.  Cannot widen further: the exact scan for rows rest[..] of the compact set's queries (wq), 8 at a time; bad[j]: where the
// compact set's query j belongs in the outputs.
static int exact_rest(const Pass& p, const std::vector<uint32_t>& rest, const std::vector<uint32_t>& bad, const uint16_t* wq, uint32_t* idx_dev,
                      int64_t* w_s, uint32_t* w_i) {
    for (size_t r0 = 0; r0 < rest.size(); r0 += 8) {
        const int nqp = (int)std::min<size_t>(8, rest.size() - r0);
        if (exact_pass(p.s, p.f, wq, rest.data() + r0, nqp, p.k, p.id_offset, w_s, w_i, (size_t)p.k)) return -1;
        std::vector<uint32_t> dst(nqp);
        for (int j = 0; j < nqp; j++) dst[j] = bad[rest[r0 + j]];
        MSE_HIP_TRY(hipMemcpyAsync(idx_dev, dst.data(), (size_t)nqp * 4, hipMemcpyHostToDevice, p.st));
        if (launch_scatter_topk(idx_dev, nullptr, nqp, p.k, w_s, w_i, p.out_scores, p.out_ids, p.out_stride, p.st)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(p.st));
    }
    return 0;
}

// Stage 4.  The queries whose certificate failed (`bad`: near-duplicate rows around their k-th score, ties) are carried on as a COMPACT
// set: their columns of the group maxima (or their lists), their query rows.  Widening then costs what those few queries cost -- not a
// 4x, 16x, 64x larger re-score for all 256 (a clustered 1e8-row set: 84 ms per pass of 256 queries instead of 58, before this).
static int widen(const Pass& p, const GroupMaxima& gm, const std::vector<uint32_t>& bad) {
    mse_searcher* s = p.s;
    hipStream_t st = p.st;
    const int k = p.k, d = p.d;
    const int nb = (int)bad.size(), nbp = (nb + 31) / 32 * 32;
    if (s->widx.ensure((size_t)nb * 5) || s->wq.ensure((size_t)(nb + 8) * d * 2) || s->wout.ensure((size_t)std::max(nb, 8) * k * 12)) return -1;
    uint32_t* idx_dev = s->widx.as<uint32_t>();
    uint8_t* take_dev = reinterpret_cast<uint8_t*>(idx_dev + nb);
    MSE_HIP_TRY(hipMemcpyAsync(idx_dev, bad.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
    if (launch_gather_rows16(p.q, (size_t)d * 2, idx_dev, nb, s->wq.p, st)) return -1;
    GroupMaxima wgm{};
    size_t most_groups = SIZE_MAX;   // the sparse form: the longest list of the compact set -- more groups than that widen nothing
    if (gm.sparse) {
        const uint32_t cap = gm.cap;
        if (s->sp_wlists.ensure((size_t)nb * 8 + (size_t)nb * cap * 8)) return -1;
        const ListSrc L = carve_lists(s->sp_wlists, nb, cap);
        if (launch_sparse_gather_lists(gm.lists.ids, gm.lists.keys, gm.lists.counts, gm.lists.tau, cap, idx_dev, nb, L.ids, L.keys, L.counts, L.tau, st)) return -1;
        most_groups = 0;
        for (uint32_t i : bad) most_groups = std::max<size_t>(most_groups, gm.counts_h[i]);
        wgm = GroupMaxima{true, nullptr, 0, L, cap, nullptr};
    } else {
        if (s->wg.ensure(p.n_groups * (size_t)nbp * 4)) return -1;
        if (launch_gather_columns(gm.dense, gm.pad, p.n_groups, idx_dev, nb, s->wg.as<float>(), nbp, st)) return -1;
        wgm = GroupMaxima{false, s->wg.as<float>(), nbp, ListSrc{}, 0, nullptr};
    }
    // (second halves of eps and margin: the compact set's)
    float* eps2 = s->eps.as<float>() + p.nq;
    float* margin2 = s->margin.as<float>() + p.nq;
    if (query_eps(p, s->wq.as<uint16_t>(), nb, eps2)) return -1;
    int64_t* w_s = s->wout.as<int64_t>();
    uint32_t* w_i = reinterpret_cast<uint32_t*>(s->wout.as<char>() + (size_t)nb * k * 8);
    const float* const margin_h = s->margin_pin.as<float>();
    std::vector<uint8_t> open_q(nb, 1);   // still uncertified
    int kg = p.kg0 * 4;
    for (;;) {
        const int kg_eff = (int)std::min<size_t>(kg, TOPK_KMAX);
        if (certified_round(p, wgm, s->wq.as<uint16_t>(), nb, kg_eff, eps2, margin2, w_s, w_i, (size_t)k)) return -1;
        // rows of the queries certified in this round (or examined completely) go to their places
        std::vector<uint8_t> take(nb, 0);
        int still = 0;
        for (int j = 0; j < nb; j++) {
            if (!open_q[j]) continue;
            if (margin_h[j] > 0.0f || (size_t)kg_eff >= p.n_groups) { take[j] = 1; open_q[j] = 0; } else still++;
        }
        MSE_HIP_TRY(hipMemcpyAsync(take_dev, take.data(), (size_t)nb, hipMemcpyHostToDevice, st));
        if (launch_scatter_topk(idx_dev, take_dev, nb, k, w_s, w_i, p.out_scores, p.out_ids, p.out_stride, st)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(st));   // `take` is a stack-owned source
        if (still == 0) return 0;
        // (a list used up leaves the threshold as the bound, which certifies by construction: the second test is a safety net that
        // sends what is still open -- a k-th score saturated to INT64_MIN, which proves nothing -- to the exact scan)
        if (kg_eff >= TOPK_KMAX || (size_t)kg_eff >= most_groups) break;
        kg = kg_eff * 4;
    }
    std::vector<uint32_t> rest;
    for (int j = 0; j < nb; j++)
        if (open_q[j]) rest.push_back((uint32_t)j);
    return exact_rest(p, rest, bad, s->wq.as<uint16_t>(), idx_dev, w_s, w_i);
}

// Stage 3.  The first round over all queries of the pass and its bookkeeping: the scan's timing, the sparse form's overflow decision
// (*overflow: a list lost survivors, nothing of this attempt stands), and who goes on to the widening.
static int first_round(const Pass& p, const GroupMaxima& gm, bool* overflow) {
    mse_searcher* s = p.s;
    if (certified_round(p, gm, p.q, p.nq, p.kg0, s->eps.as<float>(), s->margin.as<float>(), p.out_scores, p.out_ids, p.out_stride)) return -1;
    if (s->timing) {
        // (the sparse form: from the start of launch A to the end of launch B, the small kernels between them included)
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) { s->scan_ms_total += ms; s->scan_launches++; }
    }
    if (gm.sparse) {
        uint32_t longest = 0;
        for (int i = 0; i < p.nq; i++) longest = std::max(longest, gm.counts_h[i]);
        s->last_sparse_max_list = std::max(s->last_sparse_max_list, longest);
        if (longest > gm.cap) { *overflow = true; return 0; }
    }
    std::vector<uint32_t> bad;
    for (int i = 0; i < p.nq; i++)
        if (!(s->margin_pin.as<float>()[i] > 0.0f)) bad.push_back((uint32_t)i);
    if (bad.empty() || (size_t)p.kg0 >= p.n_groups) return 0;
    s->last_widened = (uint32_t)bad.size();
    return widen(p, gm, bad);
}

// The pass (the comment above Pass): what both forms of the scan need, then the sparse form where sparse_plan allows it, and the dense
// form otherwise or after an overflow.
static int mfma_pass(mse_searcher* s, const mse_filter* f, const uint16_t* q_dev, int nq_pass, int k, uint64_t id_offset,
                     int64_t* out_scores, uint32_t* out_ids, size_t out_stride) {
    const mse_base* b = s->base;
    hipStream_t st = s->stream;
    const int d = (int)b->d;
    // one pass over the rows serves up to 320 queries (padded to 128 / 192 / 256 / 320); more queries (small base only) = full passes
    // and a last one
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
    const size_t one_tile_packed = (size_t)(d / 64) * tile * 128;
    if (s->qpacked.ensure(std::max(mfma_packed_bytes(d), (size_t)std::max(n_full, 1) * one_tile_packed))) return -1;
    if (s->eps.ensure((size_t)nq_pass * 8) || s->margin.ensure((size_t)nq_pass * 8)) return -1;   // second halves: the widening's compact set
    if (s->margin_pin.ensure((size_t)nq_pass * 4, 4096)) return -1;
    s->last_widened = 0;
    const Pass p{s, b, st, f, q_dev, nq_pass, k, id_offset, out_scores, out_ids, out_stride, d, tile, n_full, rem, nq_pad, gr,
                 (b->n + gr - 1) / gr, (int)std::min<size_t>(std::max(k + 8, 16), TOPK_KMAX)};
    GroupMaxima gm{};
    SparsePlan plan;
    if (sparse_plan(s, nq_pass, k, f, &plan)) {
        bool overflow = false;
        s->last_sparse_passes++;
        if (scan_sparse(p, plan, &gm) || first_round(p, gm, &overflow)) return -1;
        if (!overflow) return 0;
        s->last_sparse_fallbacks++;
    }
    return scan_dense(p, &gm) || first_round(p, gm, nullptr) ? -1 : 0;
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

// What MSE_MODE_AUTO means for nq queries.  Answers are identical on every path.
//   any filtered call: the exact pass over the filter's id list on the sparse side of the crossover (filter_sparse), otherwise the
//     coalescer's rule with the masked matrix-core scan;
//   the coalescer (`coalesced`, dispatch.hip run_group), unfiltered: a pass of the matrix-core scan costs less than the exact-order pass
//     once the rows no longer fit the caches, whatever the query count (40 ms against 54 ms at 1e8 rows); below that the exact pass has
//     the shorter tail -- so the scan for more than 8 queries, and for any count from 2^22 rows on;
//   a direct unfiltered call: the exact pass up to its 8 queries, the scan beyond.
int bruteforce_auto_mode(const mse_base* b, const mse_filter* f, size_t nq, bool coalesced) {
    if (f && filter_sparse(b, f, nq)) return MSE_MODE_EXACT;
    if (f || coalesced) return (nq > 8 || b->n >= ((size_t)1 << 22)) ? MSE_MODE_MFMA : MSE_MODE_EXACT;
    return nq <= 8 ? MSE_MODE_EXACT : MSE_MODE_MFMA;
}

// every one of the [nq][k] output slots empty (INT64_MIN / MSE_ID_NONE)
static int fill_empty(mse_searcher* s, size_t nq, size_t k, int64_t* out_scores, uint32_t* out_ids) {
    std::vector<int64_t> hs(nq * k, INT64_MIN);
    std::vector<uint32_t> hi(nq * k, MSE_ID_NONE);
    MSE_HIP_TRY(hipMemcpyAsync(out_scores, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(out_ids, hi.data(), hi.size() * 4, hipMemcpyHostToDevice, s->stream));
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

// a searcher the brute-force search can run on: it exists and has rows behind it (a scratch searcher has none)
static int check_searcher(const mse_searcher* s) { return !s ? fail("null searcher") : !s->base ? fail("searcher has no base") : 0; }

// The one validation order of the entry points, f = null being the unfiltered and g = null the ungrouped search: -1 with the error set, 0 = nothing to do,
// 1 = go on.  (The filter before the counts: a filter that does not fit is an error even of a call that asks for nothing.)
static int check_call(const mse_searcher* s, const mse_filter* f, size_t nq, size_t k, int mode, const mse_groups* g = nullptr) {
    if (check_searcher(s)) return -1;
    if (f && check_filter(s->base, f)) return -1;
    if (g && check_groups(s->base, g)) return -1;
    if (nq == 0 || k == 0) return 0;
    if (k > (size_t)TOPK_KMAX - 64) return fail("k too large (max 1984)");
    if (mode != MSE_MODE_AUTO && mode != MSE_MODE_EXACT && mode != MSE_MODE_MFMA) return fail("unknown mode");
    return 1;
}

// a filtered entry point that was handed no filter: an error of its own, in the filter's place of the order above
static int null_filter(const mse_searcher* s) { return check_searcher(s) ? -1 : fail("null filter"); }

// The device form: [nq][d] f16 queries and [nq][k] outputs on the searcher's device.  MODE_EXACT: the exact pass (over the filter's id
// list).  MODE_MFMA: the (masked) matrix-core scan.  MODE_AUTO: bruteforce_auto_mode's direct rule.
int bruteforce_topk_dev(mse_searcher* s, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode, uint64_t id_offset,
                        void* scores_dev, void* ids_dev) {
    if (const int go = check_call(s, f, nq, k, mode); go <= 0) return go;
    const mse_base* b = s->base;
    const size_t d = b->d;
    int64_t* out_scores = reinterpret_cast<int64_t*>(scores_dev);
    uint32_t* out_ids = reinterpret_cast<uint32_t*>(ids_dev);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(queries_dev);
    s->last_widened = s->last_max_groups = 0;
    s->last_sparse_passes = s->last_sparse_fallbacks = s->last_sparse_max_list = 0;
    if (f ? f->count == 0 : b->n == 0) return fill_empty(s, nq, k, out_scores, out_ids);   // nothing allowed, or nothing to score
    if (mode == MSE_MODE_AUTO) mode = bruteforce_auto_mode(b, f, nq, false);
    const size_t tile = mode == MSE_MODE_EXACT ? 8 : mfma_call_tile(b, k);
    for (size_t q0 = 0; q0 < nq; q0 += tile) {
        const int nqp = (int)std::min<size_t>(tile, nq - q0);
        if (mode == MSE_MODE_EXACT ? exact_pass(s, f, q + q0 * d, nullptr, nqp, (int)k, id_offset, out_scores + q0 * k, out_ids + q0 * k, k)
                                   : mfma_pass(s, f, q + q0 * d, nqp, (int)k, id_offset, out_scores + q0 * k, out_ids + q0 * k, k)) return -1;
    }
    return 0;
}

// The host form.  The reference's call shape is a thread per core, each with its own Scratch and ONE query per request
// (src/query_disk_index.rs:711-736): such callers (MODE_AUTO) meet in the base's coalescer and share a pass over the rows with the
// requests of the same filter.  Answers are those of every other mode; a lone caller fires its pass at once (dispatch.h).  Only requests
// that fit one pass go there: a larger batch fills passes on its own and stays on the caller's searcher (its stream, its timing, its
// last_stats).  If the coalescer cannot be made (no memory for its worker's scratch) the call is answered directly as well.
static int bruteforce_topk_host(mse_searcher* s, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k, int mode, int64_t* scores,
                                uint32_t* ids) {
    if (const int go = check_call(s, f, nq, k, mode); go <= 0) return go;
    const size_t d = s->base->d;
    if (mode == MSE_MODE_AUTO && nq <= (size_t)mfma_query_tile((int)d)) {
        mse_dispatcher* disp = base_dispatcher(s->base);
        if (disp) return mse_dispatcher_topk_filtered_f16(disp, f, queries, nq, k, scores, ids);
    }
    DevBuf qd;
    if (qd.ensure(nq * d * 2) || s->out_scores.ensure(nq * k * 8) || s->out_ids.ensure(nq * k * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(qd.p, queries, nq * d * 2, hipMemcpyHostToDevice, s->stream));
    if (bruteforce_topk_dev(s, f, qd.p, nq, k, mode, 0, s->out_scores.p, s->out_ids.p)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(scores, s->out_scores.p, nq * k * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(ids, s->out_ids.p, nq * k * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

// ---- grouped search: one result per group (include/mse.h mse_groups) ------------------------------------------------
// a grouped entry point that was handed no grouping: an error of its own, in the grouping's place of the validation order
static int null_groups(const mse_searcher* s) { return check_searcher(s) ? -1 : fail("null grouping"); }

// The dense path for one pass of <= dense_pass_queries queries (rows pick[..] of q_dev, or its first nq_pass): the queries staged, then
// the exact pass with the grouping (exact_pass_list, which the filtered graph search's LIST regime shares), over all rows or the
// filter's id list.  Results to row dst_rows[j] (device; null: j) of the outputs.
static int grouped_dense_pass(mse_searcher* s, const mse_groups* g, const mse_filter* f, const uint16_t* q_dev, const uint32_t* pick, int nq_pass,
                              int k, uint64_t id_offset, const uint32_t* dst_rows, int64_t* out_scores, uint32_t* out_ids, size_t out_stride) {
    if (stage_exact_queries(s, q_dev, pick, nq_pass)) return -1;
    return exact_pass_list(s, nq_pass, k, id_offset, out_scores, out_ids, out_stride, f ? f->ids : nullptr, f ? f->count : s->base->n, nullptr, g,
                           dst_rows);
}

// the dense path for the nq queries at q_dev, pass by pass; results to rows dst[..] of the outputs (null: in place)
static int grouped_dense(mse_searcher* s, const mse_groups* g, const mse_filter* f, const uint16_t* q_dev, const std::vector<uint32_t>* dst, size_t nq,
                         int k, uint64_t id_offset, int64_t* out_scores, uint32_t* out_ids) {
    const size_t tile = (size_t)dense_pass_queries(g->n_rows, 12);
    if (dst && s->grp_idx.ensure(8 * 4)) return -1;
    for (size_t q0 = 0; q0 < nq; q0 += tile) {
        const int nqp = (int)std::min(tile, nq - q0);
        const uint16_t* qs = q_dev + q0 * s->base->d;
        if (!dst) {
            if (grouped_dense_pass(s, g, f, qs, nullptr, nqp, k, id_offset, nullptr, out_scores + q0 * k, out_ids + q0 * k, (size_t)k)) return -1;
            continue;
        }
        MSE_HIP_TRY(hipMemcpyAsync(s->grp_idx.p, dst->data() + q0, (size_t)nqp * 4, hipMemcpyHostToDevice, s->stream));
        if (grouped_dense_pass(s, g, f, qs, nullptr, nqp, k, id_offset, s->grp_idx.as<uint32_t>(), out_scores, out_ids, (size_t)k)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(s->stream));   // the indices are replaced by the next pass
    }
    return 0;
}

// The second half of a round of the prefix path (the first: an ordinary search for kp candidates per query into s->grp_ids [nq][kp] and
// s->grp_keys, payload key_bytes 8 = i64 or 4 = f32): the collapse of every list, and -- for the queries that are done: k representatives,
// or a list that came back short, i.e. every eligible row was seen -- the first k representatives into row dst[q] (null: q) of the
// outputs.  A prefix of the total order collapses to a prefix of the collapsed order, so these answers are exact.  open_out: the
// queries that are not done; open_reps: how many representatives each of them has so far.  Ends with the stream drained.
int grouped_collapse_round(mse_searcher* s, const mse_groups* g, int key_bytes, size_t nq, size_t kp, int k, uint64_t id_offset,
                           const std::vector<uint32_t>* dst, void* out_keys, uint32_t* out_ids, size_t out_stride, std::vector<uint32_t>* open_out,
                           std::vector<uint32_t>* open_reps) {
    hipStream_t st = s->stream;
    if (s->grp_pos.ensure(nq * k * 4) || s->grp_reps.ensure(nq * 4) || s->grp_idx.ensure(nq * 5) || s->grp_pin.ensure(nq * 8, 4096)) return -1;
    uint32_t* ids = s->grp_ids.as<uint32_t>();
    if (s->grp_timing) MSE_HIP_TRY(hipEventRecord(s->grp_ev[0], st));
    if (launch_collapse(ids, kp, kp, g->group_of, g->n_rows, k, (int)nq, s->grp_pos.as<uint32_t>(), s->grp_reps.as<uint32_t>(), st)) return -1;
    if (s->grp_timing) MSE_HIP_TRY(hipEventRecord(s->grp_ev[1], st));
    uint32_t* reps_h = s->grp_pin.as<uint32_t>();
    uint32_t* tail_h = reps_h + nq;
    MSE_HIP_TRY(hipMemcpyAsync(reps_h, s->grp_reps.p, nq * 4, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipMemcpy2DAsync(tail_h, 4, ids + (kp - 1), kp * 4, 4, nq, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (s->grp_timing) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s->grp_ev[0], s->grp_ev[1]) == hipSuccess) s->grp_ms[0] += ms;
    }
    std::vector<uint8_t> take(nq, 0);
    for (size_t i = 0; i < nq; i++) {
        if (reps_h[i] >= (uint32_t)k || tail_h[i] == ID_NONE) take[i] = 1;
        else { open_out->push_back((uint32_t)i); open_reps->push_back(reps_h[i]); }
    }
    uint32_t* dst_dev = s->grp_idx.as<uint32_t>();
    uint8_t* take_dev = reinterpret_cast<uint8_t*>(dst_dev + nq);
    if (dst) MSE_HIP_TRY(hipMemcpyAsync(dst_dev, dst->data(), nq * 4, hipMemcpyHostToDevice, st));
    MSE_HIP_TRY(hipMemcpyAsync(take_dev, take.data(), nq, hipMemcpyHostToDevice, st));
    if (launch_collapse_gather(s->grp_pos.as<uint32_t>(), k, ids, kp, s->grp_keys.p, kp, key_bytes, (int)nq, id_offset, dst ? dst_dev : nullptr,
                               take_dev, out_keys, out_ids, out_stride, st)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(st));   // `take` is a stack-owned source
    return 0;
}

// One round of the brute force's prefix path: the ordinary (masked) matrix-core search of the nq queries at qs with kp candidates each.
static int grouped_prefix_round(mse_searcher* s, const mse_groups* g, const mse_filter* f, const uint16_t* qs, size_t nq, size_t kp, int k,
                                uint64_t id_offset, const std::vector<uint32_t>* dst, int64_t* out_scores, uint32_t* out_ids,
                                std::vector<uint32_t>* open_out, std::vector<uint32_t>* open_reps) {
    if (s->grp_ids.ensure(nq * kp * 4) || s->grp_keys.ensure(nq * kp * 8)) return -1;
    if (bruteforce_topk_dev(s, f, qs, nq, kp, MSE_MODE_MFMA, 0, s->grp_keys.p, s->grp_ids.p)) return -1;
    return grouped_collapse_round(s, g, 8, nq, kp, k, id_offset, dst, out_scores, out_ids, (size_t)k, open_out, open_reps);
}

// The prefix path's rounds.  k' starts at max(2k, k + 64) -- a grouping of mean size 2 or less is done there -- and grows eightfold per
// round up to the selection limit (1984); after each round the queries still short are carried on as a COMPACT set (rows of row_bytes,
// a multiple of 16), so a longer prefix is paid for by the queries that need it only.  Eightfold: a round costs a pass over the rows plus
// a re-score that grows with k', so few rounds.  A query leaves for the dense path when the last round left it open -- or EARLY, when
// its r representatives among k' candidates say that not even 1984 will do: new groups only get rarer down the ranking, so k' x k / r
// candidates is the least it needs (a cost heuristic only: either path gives the same answer; measured at 1e7 rows, a query in a
// 99.9 % group otherwise paid three useless rounds, the last of them dearer than its dense pass).  The dense set is gathered from the
// ORIGINAL queries -- a query's output row is its index there -- and handed to `dense` with those rows.
int grouped_prefix_drive(mse_searcher* s, const void* q, size_t row_bytes, size_t nq, size_t k, const GroupedRound& round, const GroupedDense& dense) {
    const size_t k_top = (size_t)TOPK_KMAX - 64;
    size_t kp = std::min(k_top, std::max(2 * k, k + 64));
    const void* cur = q;
    size_t n_cur = nq;
    std::vector<uint32_t> rows;         // output row of each query of the current set (empty: its own index)
    std::vector<uint32_t> dense_rows;   // the queries for the dense path
    for (int r = 0;; r++) {
        std::vector<uint32_t> open, reps, go;
        if (round(cur, n_cur, kp, rows.empty() ? nullptr : &rows, &open, &reps)) return -1;
        s->last_grouped[r ? 1 : 0] += (uint32_t)(n_cur - open.size());
        for (size_t j = 0; j < open.size(); j++) {
            if (kp >= k_top || (uint64_t)kp * k > (uint64_t)k_top * std::max<uint32_t>(reps[j], 1)) dense_rows.push_back(rows.empty() ? open[j] : rows[open[j]]);
            else go.push_back(open[j]);
        }
        if (go.empty()) break;
        const size_t nb = go.size();
        DevBuf& set = (r & 1) ? s->grp_q2 : s->grp_q;   // (the current set is read while the next is written)
        if (set.ensure(nb * row_bytes) || s->grp_idx.ensure(nb * 4)) return -1;
        MSE_HIP_TRY(hipMemcpyAsync(s->grp_idx.p, go.data(), nb * 4, hipMemcpyHostToDevice, s->stream));
        if (launch_gather_rows16(cur, row_bytes, s->grp_idx.as<uint32_t>(), (int)nb, set.p, s->stream)) return -1;
        MSE_HIP_TRY(hipStreamSynchronize(s->stream));   // `go` is a stack-owned source, and grp_idx is the next round's
        for (uint32_t& j : go) j = rows.empty() ? j : rows[j];
        rows.swap(go);
        cur = set.p;
        n_cur = nb;
        kp = std::min(k_top, kp * 8);
    }
    if (dense_rows.empty()) return 0;
    const size_t nd = dense_rows.size();
    s->last_grouped[2] = (uint32_t)nd;
    if (s->grp_q.ensure(nd * row_bytes) || s->grp_idx.ensure(nd * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(s->grp_idx.p, dense_rows.data(), nd * 4, hipMemcpyHostToDevice, s->stream));
    if (launch_gather_rows16(q, row_bytes, s->grp_idx.as<uint32_t>(), (int)nd, s->grp_q.p, s->stream)) return -1;
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return dense(s->grp_q.p, nd, dense_rows);
}

// The device form of the grouped search.  MODE_EXACT: the exact pass holds every score, so the dense path at once.  MODE_MFMA: the
// prefix path (grouped_prefix_drive), the dense path for what it leaves.  MODE_AUTO: bruteforce_auto_mode's direct rule.
int grouped_topk_dev(mse_searcher* s, const mse_groups* g, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode,
                     uint64_t id_offset, void* scores_dev, void* ids_dev) {
    if (const int go = check_call(s, f, nq, k, mode, g); go <= 0) return go;
    const mse_base* b = s->base;
    int64_t* out_scores = reinterpret_cast<int64_t*>(scores_dev);
    uint32_t* out_ids = reinterpret_cast<uint32_t*>(ids_dev);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(queries_dev);
    s->last_grouped[0] = s->last_grouped[1] = s->last_grouped[2] = 0;
    const size_t eligible = f ? f->count : b->n;
    if (eligible == 0) return fill_empty(s, nq, k, out_scores, out_ids);
    if (mode == MSE_MODE_AUTO) mode = bruteforce_auto_mode(b, f, nq, false);
    if (mode == MSE_MODE_EXACT) {
        s->last_grouped[2] = (uint32_t)nq;
        return grouped_dense(s, g, f, q, nullptr, nq, (int)k, id_offset, out_scores, out_ids);
    }
    return grouped_prefix_drive(
        s, q, b->d * 2, nq, k,
        [&](const void* qs, size_t n, size_t kp, const std::vector<uint32_t>* dst, std::vector<uint32_t>* open, std::vector<uint32_t>* reps) {
            return grouped_prefix_round(s, g, f, reinterpret_cast<const uint16_t*>(qs), n, kp, (int)k, id_offset, dst, out_scores, out_ids, open, reps);
        },
        [&](const void* qs, size_t n, const std::vector<uint32_t>& dst) {
            return grouped_dense(s, g, f, reinterpret_cast<const uint16_t*>(qs), &dst, n, (int)k, id_offset, out_scores, out_ids);
        });
}

// The host form: on the caller's searcher in every mode (the base's coalescer groups requests by filter only).
static int grouped_topk_host(mse_searcher* s, const mse_groups* g, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k, int mode,
                             int64_t* scores, uint32_t* ids) {
    if (const int go = check_call(s, f, nq, k, mode, g); go <= 0) return go;
    const size_t d = s->base->d;
    DevBuf qd;
    if (qd.ensure(nq * d * 2) || s->out_scores.ensure(nq * k * 8) || s->out_ids.ensure(nq * k * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(qd.p, queries, nq * d * 2, hipMemcpyHostToDevice, s->stream));
    if (grouped_topk_dev(s, g, f, qd.p, nq, k, mode, 0, s->out_scores.p, s->out_ids.p)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(scores, s->out_scores.p, nq * k * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(ids, s->out_ids.p, nq * k * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

}  // namespace mse

using namespace mse;

extern "C" {

int mse_bruteforce_topk_f16_dev(mse_searcher* s, const void* queries_dev, size_t nq, size_t k, int mode, uint64_t id_offset, void* scores_dev, void* ids_dev) {
    return bruteforce_topk_dev(s, nullptr, queries_dev, nq, k, mode, id_offset, scores_dev, ids_dev);
}

int mse_bruteforce_topk_filtered_f16_dev(mse_searcher* s, const mse_filter* f, const void* queries_dev, size_t nq, size_t k, int mode,
                                         uint64_t id_offset, void* scores_dev, void* ids_dev) {
    if (!f) return null_filter(s);
    return bruteforce_topk_dev(s, f, queries_dev, nq, k, mode, id_offset, scores_dev, ids_dev);
}

int mse_bruteforce_topk_f16(mse_searcher* s, const uint16_t* queries, size_t nq, size_t k, int mode, int64_t* scores, uint32_t* ids) {
    return bruteforce_topk_host(s, nullptr, queries, nq, k, mode, scores, ids);
}

int mse_bruteforce_topk_filtered_f16(mse_searcher* s, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k, int mode,
                                     int64_t* scores, uint32_t* ids) {
    if (!f) return null_filter(s);
    return bruteforce_topk_host(s, f, queries, nq, k, mode, scores, ids);
}

int mse_bruteforce_topk_grouped_f16(mse_searcher* s, const mse_groups* g, const mse_filter* f, const uint16_t* queries, size_t nq, size_t k, int mode,
                                    int64_t* scores, uint32_t* ids) {
    if (!g) return null_groups(s);
    return grouped_topk_host(s, g, f, queries, nq, k, mode, scores, ids);
}

int mse_bruteforce_topk_grouped_f16_dev(mse_searcher* s, const mse_groups* g, const mse_filter* f, const void* queries_dev, size_t nq, size_t k,
                                        int mode, uint64_t id_offset, void* scores_dev, void* ids_dev) {
    if (!g) return null_groups(s);
    return grouped_topk_dev(s, g, f, queries_dev, nq, k, mode, id_offset, scores_dev, ids_dev);
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

}  // extern "C"
