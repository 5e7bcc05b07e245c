// C ABI of the descriptor pipeline over a resident index (kernels: describe.hip): the device-resident score table `mse_scores`, its exact
// order statistics and CDF fit (meme-rater/compute_cdf.py:64-71), and the in-place write of descriptor bytes into resident codes
// (src/dump_processor.rs:481-491).  Everything runs on the null stream and returns with it drained.
#include "../../include/mse.h"
#include "describe.h"
#include "index_pack.h"
#include <cmath>
#include <cstring>
#include <new>

using namespace mse;

struct mse_scores {
    int device = 0;
    size_t n = 0, n_ch = 0;
    float* scores = nullptr;     // device [n][n_ch]
    uint32_t* ts = nullptr;      // device [n] or null
    mutable std::mutex mu;       // guards the select's scratch
    mutable DevBuf sel;
};

namespace {

// mse_describe_timing: HIP-event milliseconds of the last MLP launch and of the three counting passes of the last select
std::mutex g_tm_mu;
bool g_tm_on = false;
double g_tm_mlp = 0.0, g_tm_pass[3] = {0.0, 0.0, 0.0};

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    bool on = false;
    explicit EventPair(bool enable) { on = enable && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
    void start() { if (on) (void)hipEventRecord(a, nullptr); }
    void stop() { if (on) (void)hipEventRecord(b, nullptr); }
    double ms() {   // after the stream was drained
        float t = 0.0f;
        return on && hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0;
    }
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

bool timing_on() {
    std::lock_guard<std::mutex> g(g_tm_mu);
    return g_tm_on;
}

// timestamps as the u32 channel: anything outside [0, 2^32) is refused
int upload_timestamps(const int64_t* ts, size_t n, uint32_t** out, const char* who) {
    std::vector<uint32_t> t(n);
    for (size_t i = 0; i < n; i++) {
        if (ts[i] < 0 || ts[i] > (int64_t)0xFFFFFFFFll)
            return fail(std::string(who) + ": timestamp " + std::to_string((long long)ts[i]) + " of row " + std::to_string(i) + " is outside [0, 2^32)");
        t[i] = (uint32_t)ts[i];
    }
    MSE_HIP_TRY(hipMalloc((void**)out, n * 4));
    MSE_HIP_TRY(hipMemcpy(*out, t.data(), n * 4, hipMemcpyHostToDevice));
    return 0;
}

int upload_ids(const uint32_t* ids, size_t n, size_t limit, DevBuf& buf, const char* who) {
    for (size_t i = 0; i < n; i++)
        if (ids[i] >= limit) return fail(std::string(who) + ": id " + std::to_string(ids[i]) + " at position " + std::to_string(i) + " is not below the " + std::to_string(limit) + " rows");
    if (buf.ensure(n * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(buf.p, ids, n * 4, hipMemcpyHostToDevice));
    return 0;
}

// keys_out[i] = the key at rank ranks[i] (< n) of channel `channel` (n_ch: the timestamps), at most SEL_MAX_RANKS of them
int select_chunk(const mse_scores* s, size_t channel, const uint32_t* ranks, size_t nr, uint32_t* keys_out) {
    const bool is_ts = channel == s->n_ch;
    const uint32_t* data = is_ts ? s->ts : reinterpret_cast<const uint32_t*>(s->scores) + channel;
    const size_t stride = is_ts ? 1 : s->n_ch;
    if (s->sel.ensure(SEL_SCRATCH_WORDS * 4)) return -1;
    const SelectScratch sc = select_scratch_at(s->sel.as<uint32_t>());
    MSE_HIP_TRY(hipMemsetAsync(sc.cnt1, 0, SEL_COUNTER_WORDS * 4, nullptr));
    MSE_HIP_TRY(hipMemcpyAsync(sc.rem, ranks, nr * 4, hipMemcpyHostToDevice, nullptr));
    const bool tm = timing_on();
    EventPair ev[3] = {EventPair(tm), EventPair(tm), EventPair(tm)};
    for (int pass = 1; pass <= 3; pass++) {
        ev[pass - 1].start();
        launch_select_count(pass, data, stride, s->n, is_ts ? 0 : 1, sc, nullptr);
        ev[pass - 1].stop();
        MSE_HIP_TRY(hipGetLastError());
        if (pass == 1 && !is_ts) {
            uint32_t n_nan = 0;
            MSE_HIP_TRY(hipMemcpy(&n_nan, sc.n_nan, 4, hipMemcpyDeviceToHost));
            if (n_nan) return fail("order statistics: " + std::to_string(n_nan) + " NaN among the " + std::to_string(s->n) + " keys of channel " + std::to_string(channel) + " (a NaN has no rank)");
        }
        launch_select_resolve(pass, sc, (int)nr, nullptr);
        MSE_HIP_TRY(hipGetLastError());
    }
    MSE_HIP_TRY(hipMemcpy(keys_out, sc.prefix, nr * 4, hipMemcpyDeviceToHost));
    if (tm) {
        std::lock_guard<std::mutex> g(g_tm_mu);
        for (int p = 0; p < 3; p++) g_tm_pass[p] = ev[p].ms();
    }
    return 0;
}

// out[i] = the value at rank ranks[i] as a double (exact for f32 and u32)
int order_statistics(const mse_scores* s, size_t channel, const uint64_t* ranks, size_t nr, double* out, const char* who) {
    if (channel > s->n_ch || (channel == s->n_ch && !s->ts)) return fail(std::string(who) + ": no channel " + std::to_string(channel));
    if (s->n > 0xFFFFFFFFull) return fail(std::string(who) + ": more than 2^32 - 1 keys");
    std::vector<uint32_t> r(nr), keys(nr);
    for (size_t i = 0; i < nr; i++) {
        if (ranks[i] >= s->n) return fail(std::string(who) + ": rank " + std::to_string((unsigned long long)ranks[i]) + " is not below the " + std::to_string(s->n) + " keys");
        r[i] = (uint32_t)ranks[i];
    }
    std::lock_guard<std::mutex> g(s->mu);
    MSE_HIP_TRY(hipSetDevice(s->device));
    for (size_t at = 0; at < nr; at += SEL_MAX_RANKS) {
        const size_t m = std::min<size_t>(SEL_MAX_RANKS, nr - at);
        if (select_chunk(s, channel, r.data() + at, m, keys.data() + at)) return -1;
    }
    for (size_t i = 0; i < nr; i++) {
        if (channel == s->n_ch) { out[i] = (double)keys[i]; continue; }
        const uint32_t bits = (keys[i] & 0x80000000u) ? (keys[i] & 0x7FFFFFFFu) : ~keys[i];
        float f;
        std::memcpy(&f, &bits, 4);
        out[i] = (double)f;
    }
    return 0;
}

}  // namespace

// the body of mse_scores_from_base / mse_scores_from_f16 over rows [n_rows][d] on `device` (the current one); returns drained
static mse_scores* scores_from_rows(mse_score_model* m, const uint16_t* rows_dev, size_t n_rows, size_t d, int device, const uint32_t* ids_or_null,
                                    size_t first, size_t n, const int64_t* timestamps_or_null, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    if (m->d_emb != d) { fail(who + "the model's d_emb is " + std::to_string(m->d_emb) + " but the rows have " + std::to_string(d) + " components"); return nullptr; }
    if (m->out_ch > 8) { fail(who + std::to_string(m->out_ch) + " output channels (at most 8: a descriptor has at most 8 bytes)"); return nullptr; }
    if (m->d_emb > 0x7FFFFFFFull || m->d_hidden > 0x7FFFFF00ull) { fail(who + "model too wide"); return nullptr; }
    if (!ids_or_null && (first > n_rows || n > n_rows - first)) { fail(who + "rows " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(n) + " are not within the " + std::to_string(n_rows) + " rows"); return nullptr; }
    if (n > 0x7FFFFFFFull * 128) { fail(who + "too many rows for one call"); return nullptr; }
    std::lock_guard<std::mutex> g(m->mu);
    DevBuf ids;
    if (ids_or_null && n && upload_ids(ids_or_null, n, n_rows, ids, who_c)) return nullptr;
    mse_scores* s = new (std::nothrow) mse_scores();
    if (!s) { fail("out of host memory"); return nullptr; }
    s->device = device; s->n = n; s->n_ch = m->out_ch;
    bool ok = true;
    if (n) {
        ok = hipMalloc((void**)&s->scores, n * m->out_ch * 4) == hipSuccess;
        if (!ok) fail(who + "device allocation failed");
        if (ok && timestamps_or_null) ok = upload_timestamps(timestamps_or_null, n, &s->ts, who_c) == 0;
        if (ok) {
            const bool tm = timing_on();
            EventPair ev(tm);
            ev.start();
            launch_score_mlp(rows_dev, (int)d, ids_or_null ? ids.as<uint32_t>() : nullptr, first, n, m->up, m->bias, m->down, (int)m->d_hidden,
                             (int)m->out_ch, s->scores, nullptr);
            ev.stop();
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) { ok = false; fail(who + hipGetErrorString(e)); }
            if (ok && tm) {
                std::lock_guard<std::mutex> tg(g_tm_mu);
                g_tm_mlp = ev.ms();
            }
        }
    }
    if (!ok) { mse_scores_free(s); return nullptr; }
    return s;
}

extern "C" {

mse_scores* mse_scores_from_base(mse_score_model* m, const mse_base* b, const uint32_t* ids_or_null, size_t first, size_t n,
                                 const int64_t* timestamps_or_null) {
    if (!m || !b) { fail("scores_from_base: null model or base"); return nullptr; }
    MSE_HIP_TRY_PTR(hipSetDevice(b->device));
    return scores_from_rows(m, b->dev, b->n, b->d, b->device, ids_or_null, first, n, timestamps_or_null, "scores_from_base");
}

mse_scores* mse_scores_from_f16(mse_score_model* m, const uint16_t* rows_f16, size_t n_rows, size_t d, const uint32_t* ids_or_null, size_t first,
                                size_t n, const int64_t* timestamps_or_null) {
    if (!m || (!rows_f16 && n_rows)) { fail("scores_from_f16: null model or rows"); return nullptr; }
    int device = 0;
    MSE_HIP_TRY_PTR(hipGetDevice(&device));
    DevBuf rows;
    if (rows.ensure(std::max<size_t>(n_rows * d * 2, 256))) return nullptr;
    if (n_rows * d) MSE_HIP_TRY_PTR(hipMemcpy(rows.p, rows_f16, n_rows * d * 2, hipMemcpyHostToDevice));
    return scores_from_rows(m, rows.as<uint16_t>(), n_rows, d, device, ids_or_null, first, n, timestamps_or_null, "scores_from_f16");
}

mse_scores* mse_scores_from_host(const float* scores, size_t n, size_t n_channels, const int64_t* timestamps_or_null) {
    if ((n && n_channels && !scores) || n_channels > 8) { fail("scores_from_host: null scores or more than 8 channels"); return nullptr; }
    mse_scores* s = new (std::nothrow) mse_scores();
    if (!s) { fail("out of host memory"); return nullptr; }
    s->n = n; s->n_ch = n_channels;
    bool ok = hipGetDevice(&s->device) == hipSuccess;
    if (!ok) fail("scores_from_host: no current device");
    if (ok && n && n_channels) {
        ok = hipMalloc((void**)&s->scores, n * n_channels * 4) == hipSuccess &&
             hipMemcpy(s->scores, scores, n * n_channels * 4, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) fail("scores_from_host: device allocation/copy failed");
    }
    if (ok && n && timestamps_or_null) ok = upload_timestamps(timestamps_or_null, n, &s->ts, "scores_from_host") == 0;
    if (!ok) { mse_scores_free(s); return nullptr; }
    return s;
}

void mse_scores_free(mse_scores* s) {
    if (!s) return;
    if (s->scores) (void)hipFree(s->scores);
    if (s->ts) (void)hipFree(s->ts);
    delete s;
}

size_t mse_scores_len(const mse_scores* s) { return s ? s->n : 0; }
size_t mse_scores_channels(const mse_scores* s) { return s ? s->n_ch : 0; }
int mse_scores_has_timestamps(const mse_scores* s) { return s && s->ts ? 1 : 0; }

int mse_scores_read(const mse_scores* s, float* out, uint32_t* ts_out_or_null) {
    if (!s || (!out && s->n * s->n_ch)) return fail("scores_read: null argument");
    if (ts_out_or_null && !s->ts && s->n) return fail("scores_read: the scores carry no timestamps");
    MSE_HIP_TRY(hipSetDevice(s->device));
    if (s->n * s->n_ch) MSE_HIP_TRY(hipMemcpy(out, s->scores, s->n * s->n_ch * 4, hipMemcpyDeviceToHost));
    if (ts_out_or_null && s->n) MSE_HIP_TRY(hipMemcpy(ts_out_or_null, s->ts, s->n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_scores_order_statistics(const mse_scores* s, size_t channel, const uint64_t* ranks, size_t n_ranks, double* out) {
    if (!s || (n_ranks && (!ranks || !out))) return fail("order_statistics: null argument");
    if (n_ranks == 0) return 0;
    return order_statistics(s, channel, ranks, n_ranks, out, "order_statistics");
}

int mse_scores_fit_cdfs(const mse_scores* s, size_t cdf_len, float* cdfs_out) {
    if (!s || !cdfs_out) return fail("fit_cdfs: null argument");
    if (cdf_len == 0 || cdf_len > 255) return fail("fit_cdfs: a CDF has 1 .. 255 entries (the bucket is one byte)");
    if (s->n == 0) return fail("fit_cdfs: no rows to take quantiles of");
    // numpy.quantile(x, linspace(0, 1, cdf_len)), method 'linear': v = (n - 1) q, the order statistics at floor(v) and the one after it
    const size_t L = cdf_len;
    std::vector<uint64_t> ranks(2 * L);
    std::vector<double> gamma(L), stat(2 * L);
    const double step = L > 1 ? 1.0 / (double)(L - 1) : 0.0;
    for (size_t i = 0; i < L; i++) {
        const double q = (L > 1 && i == L - 1) ? 1.0 : (double)i * step;
        const double v = (double)(s->n - 1) * q, lo = std::floor(v);
        gamma[i] = v - lo;
        ranks[i] = (uint64_t)lo;
        ranks[L + i] = std::min<uint64_t>(ranks[i] + 1, s->n - 1);
    }
    const size_t n_all = s->n_ch + (s->ts ? 1 : 0);
    for (size_t c = 0; c < n_all; c++) {
        if (order_statistics(s, c, ranks.data(), 2 * L, stat.data(), "fit_cdfs")) return -1;
        for (size_t i = 0; i < L; i++) {
            // numpy's _lerp: b - a in the type of the data (one f32 subtraction for a score channel; exact for the integer timestamps),
            // the rest in float64; then narrowed to the f32 in which IndexHeader.descriptor_cdfs is read
            const double a = stat[i], b = stat[L + i], t = gamma[i];
            const double diff = c < s->n_ch ? (double)((float)b - (float)a) : b - a;
            const double r = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
            cdfs_out[c * L + i] = (float)r;
        }
    }
    return 0;
}

int mse_codes_describe(mse_codes* c, mse_graph* graph_or_null, const mse_scores* s, const uint32_t* ids_or_null, size_t first, const float* cdfs,
                       size_t cdf_len) {
    if (!c || !s || !cdfs) return fail("codes_describe: null argument");
    if (cdf_len > 255) return fail("codes_describe: a CDF has at most 255 entries (the bucket is one byte)");
    const size_t n_desc = s->n_ch + (s->ts ? 1 : 0);
    if (c->n_desc != n_desc || !c->desc)
        return fail("codes_describe: the codes carry " + std::to_string(c->n_desc) + " descriptor bytes per row but the scores have " + std::to_string(n_desc) + " channels" + (s->ts ? " (timestamps included)" : ""));
    if (!ids_or_null && (first > c->n || s->n > c->n - first))
        return fail("codes_describe: rows " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(s->n) + " are not within the " + std::to_string(c->n) + " codes");
    if (s->n == 0) return 0;
    MSE_HIP_TRY(hipSetDevice(s->device));
    DevBuf ids, cd;
    if (ids_or_null && upload_ids(ids_or_null, s->n, c->n, ids, "codes_describe")) return -1;
    if (cd.ensure(n_desc * cdf_len * 4 + 4)) return -1;
    if (cdf_len) MSE_HIP_TRY(hipMemcpy(cd.p, cdfs, n_desc * cdf_len * 4, hipMemcpyHostToDevice));
    auto run = [&]() -> int {
        launch_describe(cd.as<float>(), (int)cdf_len, s->scores, (int)s->n_ch, s->ts, ids_or_null ? ids.as<uint32_t>() : nullptr, first, s->n, c->desc,
                        (int)n_desc, nullptr);
        MSE_HIP_TRY(hipGetLastError());
        MSE_HIP_TRY(hipStreamSynchronize(nullptr));
        return 0;
    };
    if (!graph_or_null) return run();
    // exclusive, as mse_graph_insert_rows: waits for the request-path calls in flight on the graph (they read the bytes) and keeps new ones out
    std::lock_guard<SharedExclusive> ex(graph_or_null->entry_lock);
    return run();
}

int mse_describe_timing(int enable, double* mlp_ms_or_null, double* select_pass_ms_or_null) {
    std::lock_guard<std::mutex> g(g_tm_mu);
    if (mlp_ms_or_null) *mlp_ms_or_null = g_tm_mlp;
    if (select_pass_ms_or_null) for (int p = 0; p < 3; p++) select_pass_ms_or_null[p] = g_tm_pass[p];
    g_tm_on = enable != 0;
    if (enable == 2) { g_tm_mlp = 0.0; g_tm_pass[0] = g_tm_pass[1] = g_tm_pass[2] = 0.0; }
    return 0;
}

}  // extern "C"
