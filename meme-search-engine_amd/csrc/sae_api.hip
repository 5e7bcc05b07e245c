// C ABI of the sparse-autoencoder encode over a resident index (kernels: sae.hip): the model handle `mse_sae` (sae/model.py:16-29 of the
// reference: up_proj, down_proj and the feature counters), the device-resident feature table `mse_features` (model.py:31-41 per row), its
// reconstruction and squared error (sae/train.py:55-56) and the row filter of one feature.  Everything runs on the null stream and returns
// with it drained.
#include "sae_model.h"
#include <atomic>
#include <new>
#include <unordered_map>

using namespace mse;

struct mse_features {
    uint64_t model_serial = 0;
    int device = 0;
    size_t n = 0, top_k = 0, d = 0, d_hidden = 0;
    uint32_t* counts = nullptr;  // device [n]
    uint32_t* feats = nullptr;   // device [n][top_k]
    float* acts = nullptr;       // device [n][top_k]
    uint64_t invalid = 0;
    const uint16_t* rows = nullptr;   // the source rows: borrowed from the base, or rows_owned
    uint16_t* rows_owned = nullptr;
    uint32_t* ids = nullptr;     // device [n] or null (then first + i)
    size_t first = 0;
    uint64_t row_end = 0;        // 1 + the largest source row
};

namespace {

std::atomic<uint64_t> g_serial{1};
std::mutex g_tm_mu;
bool g_tm_on = false;
double g_tm_encode = 0.0, g_tm_merge = 0.0;

std::mutex g_live_mu;
std::unordered_map<const mse_sae*, uint64_t> g_live;   // the live models and their uids (a trainer asks before it touches its model)

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

bool is_device_memory(const void* p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

float* upload_f32(const float* host, size_t count) {
    float* p = nullptr;
    if (hipMalloc((void**)&p, std::max<size_t>(count * 4, 256)) != hipSuccess) return nullptr;
    if (count && hipMemcpy(p, host, count * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return nullptr; }
    return p;
}

// the body of mse_sae_encode_base / mse_sae_encode_f16 over rows [n_rows][d] on `device` (the current one); returns drained.
// rows_owned: the table takes the rows over (and frees them on every path)
mse_features* encode_rows(mse_sae* m, const uint16_t* rows_dev, uint16_t* rows_owned, size_t n_rows, size_t d, int device, const uint32_t* ids_or_null,
                          size_t first, size_t n, int count_features, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    struct Drop { uint16_t* p; ~Drop() { if (p) (void)hipFree(p); } } drop{rows_owned};
    if (m->d_emb != d) { fail(who + "the model's d_emb is " + std::to_string(m->d_emb) + " but the rows have " + std::to_string(d) + " components"); return nullptr; }
    if (m->device != device) { fail(who + "the model lives on device " + std::to_string(m->device) + " and the rows on device " + std::to_string(device)); return nullptr; }
    if (!ids_or_null && (first > n_rows || n > n_rows - first)) { fail(who + "rows " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(n) + " are not within the " + std::to_string(n_rows) + " rows"); return nullptr; }
    if (n > 0xFFFFFFFEull) { fail(who + "too many rows for one call"); return nullptr; }
    uint64_t row_end = ids_or_null ? 0 : (n ? first + n : 0);
    if (ids_or_null)
        for (size_t i = 0; i < n; i++) {
            if (ids_or_null[i] >= n_rows) { fail(who + "id " + std::to_string(ids_or_null[i]) + " at position " + std::to_string(i) + " is not below the " + std::to_string(n_rows) + " rows"); return nullptr; }
            row_end = std::max<uint64_t>(row_end, (uint64_t)ids_or_null[i] + 1);
        }
    std::lock_guard<std::mutex> g(m->mu);
    mse_features* f = new (std::nothrow) mse_features();
    if (!f) { fail("out of host memory"); return nullptr; }
    f->model_serial = m->serial; f->device = device; f->n = n; f->top_k = m->top_k; f->d = d; f->d_hidden = m->d_hidden;
    f->rows = rows_dev; f->rows_owned = rows_owned; f->first = first; f->row_end = row_end;
    drop.p = nullptr;
    if (n == 0) return f;
    const size_t K = m->top_k, cap = sae_list_cap(K);
    auto run = [&]() -> int {
        MSE_HIP_TRY(hipMalloc((void**)&f->counts, n * 4));
        MSE_HIP_TRY(hipMalloc((void**)&f->feats, n * K * 4));
        MSE_HIP_TRY(hipMalloc((void**)&f->acts, n * K * 4));
        if (ids_or_null) {
            MSE_HIP_TRY(hipMalloc((void**)&f->ids, n * 4));
            MSE_HIP_TRY(hipMemcpy(f->ids, ids_or_null, n * 4, hipMemcpyHostToDevice));
        }
        int parts = 1, tpp = 1;
        sae_choose_parts(m, n, &parts, &tpp);
        const size_t tile_bytes = (size_t)SAE_ROW_TILE * parts * cap * 8;
        const size_t chunk_tiles = std::max<size_t>(1, SAE_LIST_BUDGET / tile_bytes);
        const size_t chunk_rows = chunk_tiles * SAE_ROW_TILE;
        const size_t pad_rows = std::min(chunk_rows, (n + SAE_ROW_TILE - 1) / SAE_ROW_TILE * SAE_ROW_TILE);
        if (m->lists.ensure(pad_rows * parts * cap * 8) || m->pcount.ensure(pad_rows * parts * 4) || m->pflag.ensure(pad_rows * parts * 4) ||
            m->misc.ensure(256))
            return -1;
        uint32_t* n_invalid = m->misc.as<uint32_t>();
        MSE_HIP_TRY(hipMemsetAsync(n_invalid, 0, 4, nullptr));
        const bool tm = [] { std::lock_guard<std::mutex> tg(g_tm_mu); return g_tm_on; }();
        double enc_ms = 0.0, mrg_ms = 0.0;
        for (size_t at = 0; at < n; at += chunk_rows) {
            const size_t cn = std::min(chunk_rows, n - at);
            EventPair ee(tm), em(tm);
            ee.start();
            launch_sae_encode(rows_dev, (int)d, f->ids ? f->ids + at : nullptr, first + at, cn, m->up, m->up_bias, (int)m->d_hidden, (int)K, parts, tpp,
                              m->lists.as<unsigned long long>(), m->pcount.as<uint32_t>(), m->pflag.as<uint32_t>(), nullptr);
            ee.stop();
            MSE_HIP_TRY(hipGetLastError());
            em.start();
            launch_sae_merge(m->lists.as<unsigned long long>(), m->pcount.as<uint32_t>(), m->pflag.as<uint32_t>(), parts, (int)K, cn, f->counts + at,
                             f->feats + at * K, f->acts + at * K, count_features ? m->counters : nullptr, n_invalid, nullptr);
            em.stop();
            MSE_HIP_TRY(hipGetLastError());
            MSE_HIP_TRY(hipStreamSynchronize(nullptr));
            enc_ms += ee.ms();
            mrg_ms += em.ms();
        }
        uint32_t inv = 0;
        MSE_HIP_TRY(hipMemcpy(&inv, n_invalid, 4, hipMemcpyDeviceToHost));
        f->invalid = inv;
        if (tm) {
            std::lock_guard<std::mutex> tg(g_tm_mu);
            g_tm_encode = enc_ms;
            g_tm_merge = mrg_ms;
        }
        return 0;
    };
    if (run()) {
        const std::string msg = mse_last_error();
        (void)hipStreamSynchronize(nullptr);
        mse_features_free(f);
        fail(who + msg);
        return nullptr;
    }
    return f;
}

}  // namespace

namespace mse {
uint64_t sae_next_serial() { return g_serial.fetch_add(1); }
bool sae_model_alive(const mse_sae* m, uint64_t uid) {
    std::lock_guard<std::mutex> g(g_live_mu);
    auto it = g_live.find(m);
    return it != g_live.end() && it->second == uid;
}
}  // namespace mse

extern "C" {

mse_sae* mse_sae_load(const float* up, const float* up_bias_or_null, const float* down, const float* down_bias_or_null, size_t d_emb,
                      size_t d_hidden, size_t top_k) {
    if (!up || !down) { fail("sae_load: null weights"); return nullptr; }
    if (d_emb < 1 || d_emb > 0x7FFFFFFFull || d_hidden < 2 || d_hidden > 0x7FFFFF00ull) { fail("sae_load: d_emb must be at least 1 and d_hidden at least 2 (and both below 2^31)"); return nullptr; }
    if (top_k < 1 || top_k > (size_t)SAE_MAX_TOP_K || top_k >= d_hidden) {
        fail("sae_load: top_k " + std::to_string(top_k) + " is not in 1 .. " + std::to_string(std::min<size_t>(SAE_MAX_TOP_K, d_hidden - 1)) + " (at most " + std::to_string(SAE_MAX_TOP_K) + " and below d_hidden = " + std::to_string(d_hidden) + ")");
        return nullptr;
    }
    mse_sae* m = new (std::nothrow) mse_sae();
    if (!m) { fail("out of host memory"); return nullptr; }
    m->serial = g_serial.fetch_add(1);
    m->uid = g_serial.fetch_add(1);
    m->d_emb = d_emb; m->d_hidden = d_hidden; m->top_k = top_k; m->n_cu = device_cu_count();
    bool ok = hipGetDevice(&m->device) == hipSuccess;
    float* down_dev = nullptr;
    if (ok) {
        m->up = upload_f32(up, d_hidden * d_emb);
        if (up_bias_or_null) m->up_bias = upload_f32(up_bias_or_null, d_hidden);
        if (down_bias_or_null) m->down_bias = upload_f32(down_bias_or_null, d_emb);
        down_dev = upload_f32(down, d_hidden * d_emb);
        ok = m->up && down_dev && (!up_bias_or_null || m->up_bias) && (!down_bias_or_null || m->down_bias) &&
             hipMalloc((void**)&m->downT, std::max<size_t>(d_hidden * d_emb * 4, 256)) == hipSuccess &&
             hipMalloc((void**)&m->counters, d_hidden * 8) == hipSuccess && hipMemset(m->counters, 0, d_hidden * 8) == hipSuccess;
    }
    if (ok) {
        launch_sae_transpose(down_dev, d_emb, d_hidden, m->downT, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
    }
    if (down_dev) (void)hipFree(down_dev);
    if (!ok) { mse_sae_free(m); fail("sae_load: device allocation/copy failed"); return nullptr; }
    { std::lock_guard<std::mutex> g(g_live_mu); g_live[m] = m->uid; }
    return m;
}

void mse_sae_free(mse_sae* m) {
    if (!m) return;
    { std::lock_guard<std::mutex> g(g_live_mu); g_live.erase(m); }
    for (void* p : {(void*)m->up, (void*)m->up_bias, (void*)m->downT, (void*)m->down_bias, (void*)m->counters})
        if (p) (void)hipFree(p);
    delete m;
}

size_t mse_sae_d_emb(const mse_sae* m) { return m ? m->d_emb : 0; }
size_t mse_sae_d_hidden(const mse_sae* m) { return m ? m->d_hidden : 0; }
size_t mse_sae_top_k(const mse_sae* m) { return m ? m->top_k : 0; }

mse_features* mse_sae_encode_base(mse_sae* m, const mse_base* b, const uint32_t* ids_or_null, size_t first, size_t n, int count_features) {
    if (!m || !b) { fail("sae_encode_base: null model or base"); return nullptr; }
    if (b->n && !is_device_memory(b->dev)) { fail("sae_encode_base: the base's rows are not device memory (a wrapped base must wrap a device pointer)"); return nullptr; }
    MSE_HIP_TRY_PTR(hipSetDevice(b->device));
    return encode_rows(m, b->dev, nullptr, b->n, b->d, b->device, ids_or_null, first, n, count_features, "sae_encode_base");
}

mse_features* mse_sae_encode_f16(mse_sae* m, const uint16_t* rows_f16, size_t n_rows, size_t d, int count_features) {
    if (!m || (!rows_f16 && n_rows)) { fail("sae_encode_f16: null model or rows"); return nullptr; }
    if (d == 0) { fail("sae_encode_f16: the rows have no components"); return nullptr; }
    int device = 0;
    MSE_HIP_TRY_PTR(hipGetDevice(&device));
    uint16_t* rows = nullptr;
    MSE_HIP_TRY_PTR(hipMalloc((void**)&rows, std::max<size_t>(n_rows * d * 2, 256)));
    if (n_rows && hipMemcpy(rows, rows_f16, n_rows * d * 2, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(rows); fail("sae_encode_f16: the upload failed"); return nullptr;
    }
    return encode_rows(m, rows, rows, n_rows, d, device, nullptr, 0, n_rows, count_features, "sae_encode_f16");
}

void mse_features_free(mse_features* f) {
    if (!f) return;
    for (void* p : {(void*)f->counts, (void*)f->feats, (void*)f->acts, (void*)f->rows_owned, (void*)f->ids})
        if (p) (void)hipFree(p);
    delete f;
}

size_t mse_features_len(const mse_features* f) { return f ? f->n : 0; }
size_t mse_features_top_k(const mse_features* f) { return f ? f->top_k : 0; }
uint64_t mse_features_invalid_rows(const mse_features* f) { return f ? f->invalid : 0; }

int mse_features_read(const mse_features* f, uint32_t* counts_or_null, uint32_t* features_or_null, float* activations_or_null) {
    if (!f) return fail("features_read: null table");
    if (f->n == 0) return 0;
    MSE_HIP_TRY(hipSetDevice(f->device));
    if (counts_or_null) MSE_HIP_TRY(hipMemcpy(counts_or_null, f->counts, f->n * 4, hipMemcpyDeviceToHost));
    if (features_or_null) MSE_HIP_TRY(hipMemcpy(features_or_null, f->feats, f->n * f->top_k * 4, hipMemcpyDeviceToHost));
    if (activations_or_null) MSE_HIP_TRY(hipMemcpy(activations_or_null, f->acts, f->n * f->top_k * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_features_reconstruct(const mse_features* f, mse_sae* m, float* recon_or_null, double* sqerr_or_null) {
    if (!f || !m) return fail("features_reconstruct: null table or model");
    if (f->model_serial != m->serial) return fail("features_reconstruct: the table was made by another model");
    if (f->n == 0 || (!recon_or_null && !sqerr_or_null)) return 0;
    MSE_HIP_TRY(hipSetDevice(f->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t d = f->d;
    const size_t chunk = recon_or_null ? std::max<size_t>(1, ((size_t)256 << 20) / (d * 4)) : f->n;
    DevBuf recon, sq;
    if (recon_or_null && recon.ensure(std::min(chunk, f->n) * d * 4)) return -1;
    if (sqerr_or_null && sq.ensure(std::min(chunk, f->n) * 8)) return -1;
    for (size_t at = 0; at < f->n; at += chunk) {
        const size_t cn = std::min(chunk, f->n - at);
        launch_sae_reconstruct(f->counts + at, f->feats + at * f->top_k, f->acts + at * f->top_k, (int)f->top_k, m->downT, m->down_bias, (int)d, f->rows,
                               f->ids ? f->ids + at : nullptr, f->first + at, cn, recon_or_null ? recon.as<float>() : nullptr,
                               sqerr_or_null ? sq.as<double>() : nullptr, nullptr);
        MSE_HIP_TRY(hipGetLastError());
        MSE_HIP_TRY(hipStreamSynchronize(nullptr));
        if (recon_or_null) MSE_HIP_TRY(hipMemcpy(recon_or_null + at * d, recon.p, cn * d * 4, hipMemcpyDeviceToHost));
        if (sqerr_or_null) MSE_HIP_TRY(hipMemcpy(sqerr_or_null + at, sq.p, cn * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

mse_filter* mse_features_filter(const mse_features* f, uint32_t feature, float min_activation, size_t n_rows) {
    if (!f) { fail("features_filter: null table"); return nullptr; }
    if (feature >= f->d_hidden) { fail("features_filter: feature " + std::to_string(feature) + " is not below d_hidden = " + std::to_string(f->d_hidden)); return nullptr; }
    if (f->row_end > n_rows) { fail("features_filter: the table speaks of row " + std::to_string(f->row_end - 1) + " but the filter has " + std::to_string(n_rows) + " rows"); return nullptr; }
    if (n_rows > 0xFFFFFFFEull) { fail("features_filter: row ids are u32: too many rows"); return nullptr; }
    if (n_rows == 0) return mse_filter_from_bits_dev(nullptr, 0);
    MSE_HIP_TRY_PTR(hipSetDevice(f->device));
    DevBuf words;
    const size_t bytes = (n_rows + 31) / 32 * 4;
    if (words.ensure(bytes)) return nullptr;
    MSE_HIP_TRY_PTR(hipMemsetAsync(words.p, 0, bytes, nullptr));
    if (f->n) {
        launch_sae_feature_bits(f->counts, f->feats, f->acts, (int)f->top_k, f->n, f->ids, f->first, feature, min_activation, words.as<uint32_t>(), nullptr);
        MSE_HIP_TRY_PTR(hipGetLastError());
    }
    MSE_HIP_TRY_PTR(hipStreamSynchronize(nullptr));
    return mse_filter_from_bits_dev(words.p, n_rows);
}

int mse_sae_counters(mse_sae* m, uint64_t* out_or_null, int reset) {
    if (!m) return fail("sae_counters: null model");
    MSE_HIP_TRY(hipSetDevice(m->device));
    std::lock_guard<std::mutex> g(m->mu);
    if (out_or_null) MSE_HIP_TRY(hipMemcpy(out_or_null, m->counters, m->d_hidden * 8, hipMemcpyDeviceToHost));
    if (reset) MSE_HIP_TRY(hipMemset(m->counters, 0, m->d_hidden * 8));
    return 0;
}

int mse_sae_set_hidden_parts(mse_sae* m, int parts) {
    if (!m) return fail("sae_set_hidden_parts: null model");
    if (parts < 0 || parts > SAE_MAX_PARTS) return fail("sae_set_hidden_parts: parts must be 0 (automatic) .. " + std::to_string(SAE_MAX_PARTS));
    std::lock_guard<std::mutex> g(m->mu);
    m->parts = parts;
    return 0;
}

int mse_sae_timing(int enable, double* encode_ms_or_null, double* merge_ms_or_null) {
    std::lock_guard<std::mutex> g(g_tm_mu);
    if (encode_ms_or_null) *encode_ms_or_null = g_tm_encode;
    if (merge_ms_or_null) *merge_ms_or_null = g_tm_merge;
    g_tm_on = enable != 0;
    if (enable == 2) g_tm_encode = g_tm_merge = 0.0;
    return 0;
}

}  // extern "C"
