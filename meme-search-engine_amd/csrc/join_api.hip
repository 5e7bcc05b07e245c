// C ABI (include/mse.h): the near-duplicate self-join of a searcher's base and the keep-first rule over its pair list; the cross join of
// a second, incoming base against it, the admission of the incoming rows and the select that packs the admitted ones.  The kernels and
// the schedule are in join.hip; the filter and the grouping a pair list yields are made by the creators of filter_api.hip / group_api.hip
// from device memory.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <cmath>
#include <new>

using namespace mse;

namespace {

constexpr uint64_t DEFAULT_CAND_CAP = (uint64_t)1 << 20;   // nominated pairs one launch may store (8 MiB)
constexpr size_t STRIP_TILES = (size_t)1 << 16;            // tiles per strip, at least one hi tile

// the confirmed pairs of a call, in arrival order: grows by doubling, contents kept
struct PairBuf {
    DevBuf buf;
    size_t cap = 0;
    int reserve(size_t pairs, size_t used, hipStream_t st) {
        if (pairs <= cap) return 0;
        const size_t want = std::max<size_t>(pairs, std::max<size_t>(2 * cap, 4096));
        DevBuf next;
        if (next.ensure(want * sizeof(JoinPair))) return -1;
        if (used) MSE_HIP_TRY(hipMemcpyAsync(next.p, buf.p, used * sizeof(JoinPair), hipMemcpyDeviceToDevice, st));
        MSE_HIP_TRY(hipStreamSynchronize(st));
        std::swap(buf.p, next.p); std::swap(buf.cap, next.cap);
        cap = want;
        return 0;
    }
};

// HIP events around a launch of the call when the measurement is on: the elapsed milliseconds are added to *into
struct PhaseTimer {
    JoinState& j; hipStream_t st; double* into;
    PhaseTimer(JoinState& js, hipStream_t stream, double* dst) : j(js), st(stream), into(dst) {
        if (j.timing && hipEventRecord(j.ev[0], st) != hipSuccess) (void)hipGetLastError();
    }
    void stop() {
        float ms = 0.0f;
        if (j.timing && hipEventRecord(j.ev[1], st) == hipSuccess && hipEventSynchronize(j.ev[1]) == hipSuccess &&
            hipEventElapsedTime(&ms, j.ev[0], j.ev[1]) == hipSuccess) *into += ms;
    }
};

void pairs_destroy(mse_pairs* p) {
    if (!p) return;
    for (void* q : {(void*)p->offsets, (void*)p->lo, (void*)p->hi, (void*)p->scores, (void*)p->rep, (void*)p->labels, (void*)p->dup_words})
        if (q) (void)hipFree(q);
    delete p;
}

// inc == null: the self-join of s's base.  Otherwise the cross join: inc's rows in the hi role (the list is a CSR over them), no window
int join_run(mse_searcher* s, const mse_base* inc, int64_t threshold, uint64_t window, const mse_filter* within, bool exact, long long eps_fix,
             uint64_t max_pairs, PairBuf& conf, uint64_t* kept_out) {
    const mse_base* b = s->base;
    JoinState& j = s->join;
    JoinStats& stt = *j.stats;
    hipStream_t st = s->stream;
    const size_t n = b->n;
    const size_t n_list = inc ? inc->n : n;          // rows the list is a CSR over
    const uint16_t* inc_rows = inc ? inc->dev : nullptr;
    const size_t n_inc = inc ? inc->n : 0;
    const int d = (int)b->d;
    const uint64_t cap = j.cand_cap ? j.cand_cap : DEFAULT_CAND_CAP;
    // threshold - bound as a double that is not above it: saturating subtraction, rounding to nearest, one step down
    const int64_t t_lo = threshold < INT64_MIN + eps_fix ? INT64_MIN : threshold - eps_fix;
    const double thr_lo = std::nextafter((double)t_lo, -INFINITY);
    if (j.cand.ensure(cap * sizeof(uint2)) || j.counters.ensure(32) || j.row_count.ensure(std::max<size_t>(n_list, 1) * 4)) return -1;
    unsigned long long* ctr = j.counters.as<unsigned long long>();   // [0] the strip's cursor, [1] tiles run, [2] pairs kept
    MSE_HIP_TRY(hipMemsetAsync(ctr, 0, 32, st));
    MSE_HIP_TRY(hipMemsetAsync(j.row_count.p, 0, std::max<size_t>(n_list, 1) * 4, st));
    const size_t n_tiles_side = (n + JOIN_TILE - 1) / JOIN_TILE;
    const size_t band = window ? (size_t)std::min<uint64_t>((window + JOIN_TILE - 1) / JOIN_TILE + 1, n_tiles_side) : n_tiles_side;
    uint64_t kept_upper = 0, nominated = 0, rescored = 0, repeats = 0;

    auto process = [&](size_t m) -> int {   // re-score cand[0 .. m)
        if (kept_upper + m > conf.cap && kept_upper) {   // what is really kept so far, before the list grows by a guess
            unsigned long long k = 0;
            MSE_HIP_TRY(hipMemcpyAsync(&k, ctr + 2, 8, hipMemcpyDeviceToHost, st));
            MSE_HIP_TRY(hipStreamSynchronize(st));
            kept_upper = std::min<uint64_t>(k, max_pairs);
        }
        const uint64_t need = std::min<uint64_t>(kept_upper + m, max_pairs);
        if (conf.reserve(std::max<size_t>((size_t)need, 1), (size_t)std::min<uint64_t>(kept_upper, conf.cap), st)) return -1;
        PhaseTimer tm(j, st, &j.ms[1]);
        if (launch_join_rescore(b->dev, inc_rows, d, j.cand.as<uint2>(), m, threshold, ctr + 2, conf.buf.as<JoinPair>(), max_pairs, j.row_count.as<uint32_t>(),
                                s->n_cu, st)) return -1;
        tm.stop();
        kept_upper = std::min<uint64_t>(kept_upper + m, max_pairs);
        rescored += m;
        return 0;
    };

    // one strip: its first launch, and -- when its nominations do not fit -- once more per window of them in tile order
    auto run_strip = [&](JoinStrip& sp, size_t n_tiles) -> int {
        if (j.tiles.ensure(n_tiles * 4) || j.tile_base.ensure(n_tiles * 8)) return -1;
        MSE_HIP_TRY(hipMemsetAsync(j.tiles.p, 0, n_tiles * 4, st));
        MSE_HIP_TRY(hipMemsetAsync(ctr, 0, 8, st));
        sp.window = window;
        sp.within = within ? within->words : nullptr; sp.within_words = within ? within->n_words : 0;
        sp.tile_count = j.tiles.as<uint32_t>();
        sp.cursor = ctr; sp.tiles_run = ctr + 1;
        sp.cand = j.cand.as<uint2>(); sp.cap = cap;
        PhaseTimer tm(j, st, &j.ms[0]);
        if (launch_join_tiles(exact, b->dev, n, inc_rows, n_inc, d, sp, threshold, thr_lo, st)) return -1;
        tm.stop();
        unsigned long long total = 0;
        MSE_HIP_TRY(hipMemcpyAsync(&total, ctr, 8, hipMemcpyDeviceToHost, st));
        MSE_HIP_TRY(hipStreamSynchronize(st));
        nominated += total;
        if (total <= cap) return process((size_t)total);
        if (launch_join_scan_tiles(sp.tile_count, n_tiles, j.tile_base.as<unsigned long long>(), st)) return -1;
        sp.tile_base = j.tile_base.as<unsigned long long>();
        for (unsigned long long w = 0; w < total; w += cap) {
            sp.win_lo = w;
            PhaseTimer tw(j, st, &j.ms[0]);
            if (launch_join_tiles(exact, b->dev, n, inc_rows, n_inc, d, sp, threshold, thr_lo, st)) return -1;
            tw.stop();
            if (process((size_t)std::min<unsigned long long>(cap, total - w))) return -1;
            repeats++;
        }
        return 0;
    };

    if (inc) {
        // the rectangle: a strip is a run of base tiles (y) by a run of incoming tiles (x, fastest); all incoming tiles when they fit, so the
        // base streams once per strip while the incoming panel is re-read from L2
        const size_t inc_tiles = (n_inc + JOIN_TILE - 1) / JOIN_TILE;
        for (size_t x0 = 0; x0 < inc_tiles; x0 += STRIP_TILES) {
            const size_t span = std::min(inc_tiles - x0, STRIP_TILES);
            const size_t rows_y = std::min<size_t>(std::max<size_t>(STRIP_TILES / span, 1), 65535);
            for (size_t h0 = 0; h0 < n_tiles_side; h0 += rows_y) {
                JoinStrip sp;
                sp.h0 = (uint32_t)h0; sp.n_hi = (uint32_t)std::min(rows_y, n_tiles_side - h0); sp.span = (uint32_t)span; sp.x0 = (uint32_t)x0;
                if (run_strip(sp, (size_t)sp.n_hi * span)) return -1;
            }
        }
    }
    for (size_t h0 = 0; !inc && h0 < n_tiles_side;) {
        // hi tiles of this strip: as many as keep it within STRIP_TILES tiles
        size_t n_hi = 1;
        auto span_of = [&](size_t last) { return std::min(last + 1, band); };
        while (h0 + n_hi < n_tiles_side && n_hi < 65535 && (n_hi + 1) * span_of(h0 + n_hi) <= STRIP_TILES) n_hi++;
        const size_t span = span_of(h0 + n_hi - 1);
        JoinStrip sp;
        sp.h0 = (uint32_t)h0; sp.n_hi = (uint32_t)n_hi; sp.span = (uint32_t)span;
        if (run_strip(sp, n_hi * span)) return -1;
        h0 += n_hi;
    }
    unsigned long long fin[3] = {0, 0, 0};
    MSE_HIP_TRY(hipMemcpyAsync(fin, ctr, 24, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    stt.v[0] = fin[1]; stt.v[1] = nominated; stt.v[2] = rescored; stt.v[3] = fin[2]; stt.v[4] = repeats;
    *kept_out = fin[2];
    return 0;
}

// the confirmed pairs of a finished join_run as a list in canonical order (a CSR over n_rows hi rows)
mse_pairs* make_list(mse_searcher* s, int kind, size_t n_rows, size_t base_rows, PairBuf& conf, uint64_t kept, const char* who) {
    mse_pairs* p = new (std::nothrow) mse_pairs();
    if (!p) { fail("out of host memory"); return nullptr; }
    p->device = s->base->device; p->kind = kind; p->n_rows = n_rows; p->base_rows = base_rows; p->count = (size_t)kept; p->stats = s->join.stats;
    const size_t c1 = std::max<size_t>(p->count, 1);
    bool ok = hipMalloc((void**)&p->offsets, (p->n_rows + 1) * 8) == hipSuccess && hipMalloc((void**)&p->lo, c1 * 4) == hipSuccess &&
              hipMalloc((void**)&p->hi, c1 * 4) == hipSuccess && hipMalloc((void**)&p->scores, c1 * 8) == hipSuccess;
    if (!ok) fail("hipMalloc failed for the pair list");
    PhaseTimer tm(s->join, s->stream, &s->join.ms[2]);
    ok = ok && launch_join_csr(conf.buf.as<JoinPair>(), p->count, p->n_rows, s->join.row_count.as<uint32_t>(), p->offsets, p->lo, p->hi, p->scores,
                               s->stream) == 0;
    if (ok) tm.stop();
    if (ok && hipStreamSynchronize(s->stream) != hipSuccess) { ok = false; fail(std::string(who) + ": building the list failed"); }
    if (!ok) { (void)hipStreamSynchronize(s->stream); pairs_destroy(p); return nullptr; }
    return p;
}

// the keep-first rule over p's list, once: rounds until no row is open, then representatives, the dropped rows' bitmap and the labels
int resolve(mse_pairs* p) {
    std::lock_guard<std::mutex> g(p->mu);
    if (p->resolved) return 0;
    const size_t n = p->n_rows, n1 = std::max<size_t>(n, 1);
    const size_t dup_words = (n + 255) / 256 * 8;
    DevBuf a, b, ctr, member;
    if (a.ensure(n1) || b.ensure(n1) || ctr.ensure(8) || member.ensure(n1)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(a.p, 0, n1, nullptr));
    MSE_HIP_TRY(hipMemsetAsync(member.p, 0, n1, nullptr));
    uint64_t rounds = 0;
    uint8_t *in = a.as<uint8_t>(), *out = b.as<uint8_t>();
    for (unsigned long long open = n; open != 0;) {
        MSE_HIP_TRY(hipMemsetAsync(ctr.p, 0, 8, nullptr));
        if (launch_join_round(p->offsets, p->lo, n, in, out, ctr.as<unsigned long long>(), nullptr)) return -1;
        unsigned long long now = 0;
        MSE_HIP_TRY(hipMemcpy(&now, ctr.p, 8, hipMemcpyDeviceToHost));
        if (now >= open && rounds) return fail("pairs: the keep-first rounds made no progress");   // (cannot happen: the lowest open row decides)
        open = now;
        std::swap(in, out);
        rounds++;
    }
    uint32_t *rep = nullptr, *labels = nullptr, *dup = nullptr;
    bool ok = hipMalloc((void**)&rep, n1 * 4) == hipSuccess && hipMalloc((void**)&labels, n1 * 4) == hipSuccess &&
              hipMalloc((void**)&dup, std::max<size_t>(dup_words, 1) * 4) == hipSuccess;
    if (!ok) fail("hipMalloc failed for the pair list's resolution");
    ok = ok && launch_join_finish(p->offsets, p->lo, n, in, rep, member.as<uint8_t>(), dup, labels, nullptr) == 0;
    if (ok && hipStreamSynchronize(nullptr) != hipSuccess) { ok = false; fail("pairs: the resolution failed"); }
    if (!ok) {
        for (void* q : {(void*)rep, (void*)labels, (void*)dup}) if (q) (void)hipFree(q);
        return -1;
    }
    p->rep = rep; p->labels = labels; p->dup_words = dup;
    p->rounds = rounds;
    p->resolved = true;
    return 0;
}

// resolve under p's device, and the rounds into the stats of the searcher that made p
int resolved_on_device(const mse_pairs* cp, const char* who) {
    if (!cp) return fail(std::string(who) + ": null pair list");
    if (cp->kind != 0)   // keep-first over a cross list needs the resident rows first and all kept: that rule is mse_pairs_admit
        return fail(std::string(who) + ": the list is a cross list (base rows against incoming rows); its keep-first rule is mse_pairs_admit");
    mse_pairs* p = const_cast<mse_pairs*>(cp);   // the resolution is a cache behind an immutable list
    if (hipSetDevice(p->device) != hipSuccess) return fail(std::string(who) + ": hipSetDevice failed");
    if (resolve(p)) return -1;
    if (p->stats) p->stats->v[5] = p->rounds;
    return 0;
}

}  // namespace

extern "C" {

mse_pairs* mse_join_self(mse_searcher* s, int64_t threshold, uint64_t window, const mse_filter* within, int mode, uint64_t max_pairs) {
    if (!s || !s->base) { fail("join_self: null searcher"); return nullptr; }
    const mse_base* b = s->base;
    if (within && check_filter(b, within)) return nullptr;
    if (mode != MSE_MODE_AUTO && mode != MSE_MODE_EXACT && mode != MSE_MODE_MFMA) { fail("unknown mode"); return nullptr; }
    if (b->n > 0xFFFFFFFEull) { fail("row ids are u32: too many rows"); return nullptr; }
    if (b->n && (b->d % 32 || b->d > (size_t)D_MAX)) { fail("join_self: vector width must be a multiple of 32"); return nullptr; }
    if (hipSetDevice(b->device) != hipSuccess) { fail("join_self: hipSetDevice failed"); return nullptr; }
    for (auto& v : s->join.stats->v) v = 0;
    for (double& m : s->join.ms) m = 0.0;
    long long eps_fix = 0;
    if (mode != MSE_MODE_EXACT && b->n && mfma_pair_bound(b, s->stream, &eps_fix)) return nullptr;
    const bool exact = mode == MSE_MODE_EXACT || eps_fix == 0;   // no bound can be stated: the exact path

    PairBuf conf;
    uint64_t kept = 0;
    if (join_run(s, nullptr, threshold, window, within, exact, eps_fix, max_pairs, conf, &kept)) { (void)hipStreamSynchronize(s->stream); return nullptr; }
    if (kept > max_pairs) {
        fail("join_self: " + std::to_string(kept) + " pairs reach the threshold, max_pairs is " + std::to_string(max_pairs));
        return nullptr;
    }
    return make_list(s, 0, b->n, b->n, conf, kept, "join_self");
}

mse_pairs* mse_join_cross(mse_searcher* s, const mse_base* incoming, int64_t threshold, const mse_filter* within, int mode, uint64_t max_pairs) {
    if (!s || !s->base) { fail("join_cross: null searcher"); return nullptr; }
    if (!incoming) { fail("join_cross: null incoming base"); return nullptr; }
    const mse_base* b = s->base;
    if (incoming->d != b->d) {
        fail("join_cross: the incoming rows are " + std::to_string(incoming->d) + " wide, the base's " + std::to_string(b->d));
        return nullptr;
    }
    if (incoming->device != b->device) { fail("join_cross: the incoming base is on another device than the resident one"); return nullptr; }
    if (within && check_filter(b, within)) return nullptr;
    if (mode != MSE_MODE_AUTO && mode != MSE_MODE_EXACT && mode != MSE_MODE_MFMA) { fail("unknown mode"); return nullptr; }
    if (b->n > 0xFFFFFFFEull || incoming->n > 0xFFFFFFFEull) { fail("row ids are u32: too many rows"); return nullptr; }
    if (b->d % 32 || b->d > (size_t)D_MAX) { fail("join_cross: vector width must be a multiple of 32"); return nullptr; }
    if (hipSetDevice(b->device) != hipSuccess) { fail("join_cross: hipSetDevice failed"); return nullptr; }
    for (auto& v : s->join.stats->v) v = 0;
    for (double& ms : s->join.ms) ms = 0.0;
    const bool empty = b->n == 0 || incoming->n == 0;
    long long eps_fix = 0;
    if (mode != MSE_MODE_EXACT && !empty && mfma_cross_bound(b, incoming, s->stream, &eps_fix)) return nullptr;
    const bool exact = mode == MSE_MODE_EXACT || eps_fix == 0;   // no bound can be stated for a pair of the two bases: the exact path

    PairBuf conf;
    uint64_t kept = 0;
    // (a rectangle with an empty side has no tile: join_run then only zeroes the row counts the list is built from)
    if (join_run(s, incoming, threshold, 0, within, exact, eps_fix, max_pairs, conf, &kept)) { (void)hipStreamSynchronize(s->stream); return nullptr; }
    if (kept > max_pairs) {
        fail("join_cross: " + std::to_string(kept) + " pairs reach the threshold, max_pairs is " + std::to_string(max_pairs));
        return nullptr;
    }
    return make_list(s, 1, incoming->n, b->n, conf, kept, "join_cross");
}

void mse_pairs_free(mse_pairs* p) { pairs_destroy(p); }
size_t mse_pairs_rows(const mse_pairs* p) { return p ? p->n_rows : 0; }
size_t mse_pairs_count(const mse_pairs* p) { return p ? p->count : 0; }
int mse_pairs_kind(const mse_pairs* p) { return p ? p->kind : 0; }
size_t mse_pairs_base_rows(const mse_pairs* p) { return p ? p->base_rows : 0; }

int mse_pairs_read(const mse_pairs* p, size_t first, size_t n, uint32_t* lo, uint32_t* hi, int64_t* scores) {
    if (!p) return fail("pairs_read: null pair list");
    if (first > p->count || n > p->count - first)
        return fail("pairs_read: [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") is past the list's " +
                    std::to_string(p->count) + " pairs");
    if (n == 0) return 0;
    if (lo && hipMemcpy(lo, p->lo + first, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("pairs_read: the read-back failed");
    if (hi && hipMemcpy(hi, p->hi + first, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("pairs_read: the read-back failed");
    if (scores && hipMemcpy(scores, p->scores + first, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("pairs_read: the read-back failed");
    return 0;
}

int mse_join_stats(const mse_searcher* s, uint64_t out[6]) {
    if (!s || !out) return fail("null argument");
    for (int i = 0; i < 6; i++) out[i] = s->join.stats->v[i];
    return 0;
}

int mse_join_timing(mse_searcher* s, int enable, double out[3]) {
    if (!s) return fail("null searcher");
    for (int i = 0; out && i < 3; i++) out[i] = s->join.ms[i];
    for (int i = 0; enable && i < 2; i++)
        if (!s->join.ev[i]) MSE_HIP_TRY(hipEventCreate(&s->join.ev[i]));
    s->join.timing = enable != 0;
    return 0;
}

int mse_debug_join_candidate_capacity(mse_searcher* s, uint64_t n) {
    if (!s) return fail("null searcher");
    if (n > ((uint64_t)1 << 28)) return fail("join candidate capacity: at most 2^28 pairs");
    s->join.cand_cap = n;   // 0: the default
    return 0;
}

mse_filter* mse_pairs_duplicates(const mse_pairs* p) {
    if (resolved_on_device(p, "pairs_duplicates")) return nullptr;
    return mse_filter_from_bits_dev(p->n_rows ? p->dup_words : nullptr, p->n_rows);
}

mse_groups* mse_pairs_groups(const mse_pairs* p) {
    if (resolved_on_device(p, "pairs_groups")) return nullptr;
    return mse_groups_from_dev(p->n_rows ? p->labels : nullptr, p->n_rows);
}

int mse_pairs_representatives(const mse_pairs* p, uint32_t* rep) {
    if (resolved_on_device(p, "pairs_representatives")) return -1;
    if (p->n_rows == 0) return 0;
    if (!rep) return fail("pairs_representatives: null buffer");
    if (hipMemcpy(rep, p->rep, p->n_rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("pairs_representatives: the read-back failed");
    return 0;
}

int mse_pairs_admit(const mse_pairs* cross, const mse_pairs* among, mse_filter** kept_out, uint32_t* rep_base, uint32_t* rep_incoming) {
    if (!cross) return fail("pairs_admit: null pair list");
    if (cross->kind != 1) return fail("pairs_admit: the first list must be a cross list (mse_join_cross)");
    if (among && among->kind != 0) return fail("pairs_admit: the list among the incoming rows must be a self list (mse_join_self)");
    if (among && among->n_rows != cross->n_rows)
        return fail("pairs_admit: the self list is over " + std::to_string(among->n_rows) + " rows, the cross list over " +
                    std::to_string(cross->n_rows) + " incoming rows");
    if (among && among->device != cross->device) return fail("pairs_admit: the two lists are on different devices");
    if (!kept_out) return fail("pairs_admit: null kept_out");
    *kept_out = nullptr;
    if (hipSetDevice(cross->device) != hipSuccess) return fail("pairs_admit: hipSetDevice failed");
    const size_t m = cross->n_rows, m1 = std::max<size_t>(m, 1);
    const size_t kept_words = (m + 255) / 256 * 8;
    DevBuf a, b, ctr, reps, words;
    if (a.ensure(m1) || b.ensure(m1) || ctr.ensure(8) || reps.ensure(m1 * 8) || words.ensure(std::max<size_t>(kept_words, 1) * 4)) return -1;
    uint8_t *in = a.as<uint8_t>(), *out = b.as<uint8_t>();
    // rows with a cross pair are dropped before the first round: the resident rows come first in the walk and are all kept
    MSE_HIP_TRY(hipMemsetAsync(ctr.p, 0, 8, nullptr));
    if (launch_join_admit_init(cross->offsets, m, among == nullptr, in, ctr.as<unsigned long long>(), nullptr)) return -1;
    unsigned long long open = 0;
    MSE_HIP_TRY(hipMemcpy(&open, ctr.p, 8, hipMemcpyDeviceToHost));
    uint64_t rounds = 0;
    while (open != 0) {
        MSE_HIP_TRY(hipMemsetAsync(ctr.p, 0, 8, nullptr));
        if (launch_join_round(among->offsets, among->lo, m, in, out, ctr.as<unsigned long long>(), nullptr)) return -1;
        unsigned long long now = 0;
        MSE_HIP_TRY(hipMemcpy(&now, ctr.p, 8, hipMemcpyDeviceToHost));
        if (now >= open) return fail("pairs_admit: the keep-first rounds made no progress");   // (cannot happen: the lowest open row decides)
        open = now;
        std::swap(in, out);
        rounds++;
    }
    uint32_t* rb = reps.as<uint32_t>();
    if (launch_join_admit_finish(cross->offsets, cross->lo, among ? among->offsets : nullptr, among ? among->lo : nullptr, m, in, rb, rb + m1,
                                 words.as<uint32_t>(), nullptr)) return -1;
    if (m && rep_base) MSE_HIP_TRY(hipMemcpy(rep_base, rb, m * 4, hipMemcpyDeviceToHost));
    if (m && rep_incoming) MSE_HIP_TRY(hipMemcpy(rep_incoming, rb + m1, m * 4, hipMemcpyDeviceToHost));
    mse_filter* f = mse_filter_from_bits_dev(m ? words.p : nullptr, m);
    if (!f) return -1;
    if (cross->stats) cross->stats->v[5] = rounds;
    *kept_out = f;
    return 0;
}

}  // extern "C"
