// C ABI of sparse-autoencoder training over a resident index (kernels: sae_train.hip; the forward pass: sae.hip): the handle
// `mse_sae_trainer` over an `mse_sae`, whose device weights it updates in place (sae/train.py:51-59 of the reference).  A call of many
// steps is queued whole on the null stream -- the gate is a device flag -- and returns with the stream drained.
#include "sae_model.h"
#include "sae_train.h"
#include <cmath>
#include <new>

using namespace mse;

struct mse_sae_trainer {
    mse_sae* model = nullptr;
    uint64_t model_uid = 0;
    int device = 0;
    double lr = 0, beta1 = 0, beta2 = 0, eps = 0, wd = 0;
    uint64_t t = 0;              // completed steps since the moments were zero (or since state_write)
    int skip = 1;
    float *m_up = nullptr, *v_up = nullptr, *m_down = nullptr, *v_down = nullptr;   // [d_hidden][d_emb]
    float *m_ub = nullptr, *v_ub = nullptr, *m_db = nullptr, *v_db = nullptr;       // [d_hidden] (with an encoder bias), [d_emb]
    uint2* fmap = nullptr;       // [d_hidden], {0, 0} between steps
    uint8_t* touched = nullptr;  // [d_hidden]
    DevBuf counts, feats, acts, recon, sqerr, gR, p_row, p_feat, p_act, p_h, ids, rows, losses, hyper, ctl;
};

namespace {

std::mutex g_tm_mu;
bool g_tm_on = false;
double g_tm[4] = {0.0, 0.0, 0.0, 0.0};   // forward, backward, update milliseconds and the steps they cover

bool is_device_pointer(const void* p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

float* zeros_f32(size_t count) {
    float* p = nullptr;
    const size_t bytes = std::max<size_t>(count * 4, 256);
    if (hipMalloc((void**)&p, bytes) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, bytes) != hipSuccess) { (void)hipFree(p); return nullptr; }
    return p;
}

int check_trainer(const mse_sae_trainer* tr, const char* who) {
    if (!tr) return fail(std::string(who) + ": null trainer");
    if (!sae_model_alive(tr->model, tr->model_uid)) return fail(std::string(who) + ": the trainer's model has been freed");
    return 0;
}

// n_steps steps of `batch` rows: step s takes rows ids[s batch + i] (device ids) or, ids null, rows s batch + i of `rows`
int run_steps(mse_sae_trainer* tr, const uint16_t* rows, const uint32_t* ids_dev, size_t batch, size_t n_steps, double* losses_out,
              size_t* steps_done_out) {
    mse_sae* m = tr->model;
    const size_t B = batch, E = m->d_emb, H = m->d_hidden, K = m->top_k, cap = sae_list_cap(K);
    std::lock_guard<std::mutex> g(m->mu);
    m->serial = sae_next_serial();   // a table made before this call is no longer this model's
    if (tr->counts.ensure(B * 4) || tr->feats.ensure(B * K * 4) || tr->acts.ensure(B * K * 4) || tr->recon.ensure(B * E * 4) ||
        tr->sqerr.ensure(B * 8) || tr->gR.ensure(B * E * 4) || tr->p_row.ensure(B * K * 4) || tr->p_feat.ensure(B * K * 4) ||
        tr->p_act.ensure(B * K * 4) || tr->p_h.ensure(B * K * 4) || tr->losses.ensure(n_steps * 8) ||
        tr->hyper.ensure(n_steps * sizeof(SaeAdamStep)) || tr->ctl.ensure(256))
        return -1;
    int parts = 1, tpp = 1;
    sae_choose_parts(m, B, &parts, &tpp);
    const size_t tile_bytes = (size_t)SAE_ROW_TILE * parts * cap * 8;
    const size_t chunk_rows = std::max<size_t>(1, SAE_LIST_BUDGET / tile_bytes) * SAE_ROW_TILE;
    const size_t pad_rows = std::min(chunk_rows, (B + SAE_ROW_TILE - 1) / SAE_ROW_TILE * SAE_ROW_TILE);
    if (m->lists.ensure(pad_rows * parts * cap * 8) || m->pcount.ensure(pad_rows * parts * 4) || m->pflag.ensure(pad_rows * parts * 4)) return -1;
    std::vector<SaeAdamStep> hyper(n_steps);
    for (size_t s = 0; s < n_steps; s++) {
        const double t = (double)(tr->t + s + 1);
        hyper[s].decay = (float)(1.0 - tr->lr * tr->wd);
        hyper[s].step_size = (float)(tr->lr / (1.0 - std::pow(tr->beta1, t)));
        hyper[s].bc2_sqrt = (float)std::sqrt(1.0 - std::pow(tr->beta2, t));
    }
    MSE_HIP_TRY(hipMemcpy(tr->hyper.p, hyper.data(), n_steps * sizeof(SaeAdamStep), hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemsetAsync(tr->ctl.p, 0, sizeof(SaeTrainCtl), nullptr));
    const bool tm = [] { std::lock_guard<std::mutex> tg(g_tm_mu); return g_tm_on; }();
    std::vector<hipEvent_t> ev;
    struct DropEvents { std::vector<hipEvent_t>& e; ~DropEvents() { for (hipEvent_t x : e) (void)hipEventDestroy(x); } } drop{ev};
    if (tm) {
        ev.reserve(4 * n_steps);
        for (size_t i = 0; i < 4 * n_steps; i++) {
            hipEvent_t e = nullptr;
            MSE_HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
    }
    SaeTrainStep st{};
    st.ctl = tr->ctl.as<SaeTrainCtl>();
    st.adam = SaeAdam{(float)tr->beta1, (float)tr->beta2, (float)tr->eps};
    st.B = (int)B; st.E = (int)E; st.H = (int)H; st.K = (int)K;
    st.counts = tr->counts.as<uint32_t>(); st.feats = tr->feats.as<uint32_t>(); st.acts = tr->acts.as<float>(); st.recon = tr->recon.as<float>();
    st.sqerr = tr->sqerr.as<double>(); st.rows = rows;
    st.gR = tr->gR.as<float>(); st.p_row = tr->p_row.as<uint32_t>(); st.p_feat = tr->p_feat.as<uint32_t>(); st.p_act = tr->p_act.as<float>();
    st.p_h = tr->p_h.as<float>(); st.fmap = tr->fmap; st.touched = tr->touched;
    st.skip = tr->skip && hyper[0].decay == 1.0f && st.adam.eps > 0.0f;
    st.up = m->up; st.m_up = tr->m_up; st.v_up = tr->v_up; st.downT = m->downT; st.m_down = tr->m_down; st.v_down = tr->v_down;
    st.up_bias = m->up_bias; st.m_ub = tr->m_ub; st.v_ub = tr->v_ub; st.down_bias = m->down_bias; st.m_db = tr->m_db; st.v_db = tr->v_db;
    st.counters = m->counters; st.n_cu = m->n_cu;
    uint32_t* const n_invalid = &st.ctl->n_invalid;
    auto queue = [&]() -> int {
        for (size_t s = 0; s < n_steps; s++) {
            st.hyper = tr->hyper.as<SaeAdamStep>() + s;
            st.loss = tr->losses.as<double>() + s;
            st.ids = ids_dev ? ids_dev + s * B : nullptr;
            st.first = ids_dev ? 0 : s * B;
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s], nullptr));
            for (size_t at = 0; at < B; at += chunk_rows) {
                const size_t cn = std::min(chunk_rows, B - at);
                launch_sae_encode(rows, (int)E, st.ids ? st.ids + at : nullptr, st.first + at, cn, m->up, m->up_bias, (int)H, (int)K, parts, tpp,
                                  m->lists.as<unsigned long long>(), m->pcount.as<uint32_t>(), m->pflag.as<uint32_t>(), nullptr);
                launch_sae_merge(m->lists.as<unsigned long long>(), m->pcount.as<uint32_t>(), m->pflag.as<uint32_t>(), parts, (int)K, cn,
                                 tr->counts.as<uint32_t>() + at, tr->feats.as<uint32_t>() + at * K, tr->acts.as<float>() + at * K, nullptr, n_invalid,
                                 nullptr);
            }
            launch_sae_reconstruct(st.counts, st.feats, st.acts, (int)K, m->downT, m->down_bias, (int)E, rows, st.ids, st.first, B, tr->recon.as<float>(),
                                   tr->sqerr.as<double>(), nullptr);
            launch_sae_train_gate(st, nullptr);
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s + 1], nullptr));
            launch_sae_train_backward(st, nullptr);
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s + 2], nullptr));
            launch_sae_train_update(st, nullptr);
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s + 3], nullptr));
            MSE_HIP_TRY(hipGetLastError());
        }
        return 0;
    };
    const int rc = queue();
    if (hipStreamSynchronize(nullptr) != hipSuccess && rc == 0) return fail("sae_trainer_steps: the device reported an error");
    SaeTrainCtl ctl{};
    MSE_HIP_TRY(hipMemcpy(&ctl, tr->ctl.p, sizeof ctl, hipMemcpyDeviceToHost));
    const size_t done = std::min<size_t>(ctl.steps_done, n_steps);
    tr->t += done;
    if (steps_done_out) *steps_done_out = done;
    if (rc) return -1;
    if (losses_out && done) MSE_HIP_TRY(hipMemcpy(losses_out, tr->losses.p, done * 8, hipMemcpyDeviceToHost));
    if (tm) {
        double f = 0.0, b = 0.0, u = 0.0;
        for (size_t s = 0; s < done; s++) {
            float x = 0.0f;
            if (hipEventElapsedTime(&x, ev[4 * s], ev[4 * s + 1]) == hipSuccess) f += x;
            if (hipEventElapsedTime(&x, ev[4 * s + 1], ev[4 * s + 2]) == hipSuccess) b += x;
            if (hipEventElapsedTime(&x, ev[4 * s + 2], ev[4 * s + 3]) == hipSuccess) u += x;
        }
        std::lock_guard<std::mutex> tg(g_tm_mu);
        g_tm[0] = f; g_tm[1] = b; g_tm[2] = u; g_tm[3] = (double)done;
    }
    return 0;
}

int check_call(const mse_sae_trainer* tr, size_t d, int device, size_t batch, size_t n_steps, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    const mse_sae* m = tr->model;
    if (m->d_emb != d) return fail(who + "the model's d_emb is " + std::to_string(m->d_emb) + " but the rows have " + std::to_string(d) + " components");
    if (m->device != device) return fail(who + "the model lives on device " + std::to_string(m->device) + " and the rows on device " + std::to_string(device));
    if (batch == 0) return fail(who + "an empty batch");
    if (batch > SAE_TRAIN_MAX_PAIRS || batch * m->top_k > SAE_TRAIN_MAX_PAIRS)
        return fail(who + "batch * top_k = " + std::to_string(batch) + " * " + std::to_string(m->top_k) + " exceeds " + std::to_string(SAE_TRAIN_MAX_PAIRS));
    if (n_steps > 0xFFFFFFFFull / batch) return fail(who + "too many rows for one call");
    return 0;
}

}  // namespace

extern "C" {

mse_sae_trainer* mse_sae_trainer_create(mse_sae* m, double lr, double beta1, double beta2, double eps, double weight_decay) {
    if (!m) { fail("sae_trainer_create: null model"); return nullptr; }
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(lr >= 0.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) ||
        !std::isfinite(lr) || !std::isfinite(eps) || !std::isfinite(weight_decay)) {
        fail("sae_trainer_create: invalid AdamW parameters");
        return nullptr;
    }
    if (!m->down_bias) { fail("sae_trainer_create: the model has no down_bias (the reference's decoder always has one: load a zero vector)"); return nullptr; }
    if (m->d_emb > ((size_t)1 << 24)) { fail("sae_trainer_create: d_emb above 2^24"); return nullptr; }
    MSE_HIP_TRY_PTR(hipSetDevice(m->device));
    mse_sae_trainer* tr = new (std::nothrow) mse_sae_trainer();
    if (!tr) { fail("out of host memory"); return nullptr; }
    tr->model = m; tr->model_uid = m->uid; tr->device = m->device;
    tr->lr = lr; tr->beta1 = beta1; tr->beta2 = beta2; tr->eps = eps; tr->wd = weight_decay;
    const size_t he = m->d_hidden * m->d_emb;
    tr->m_up = zeros_f32(he); tr->v_up = zeros_f32(he); tr->m_down = zeros_f32(he); tr->v_down = zeros_f32(he);
    tr->m_db = zeros_f32(m->d_emb); tr->v_db = zeros_f32(m->d_emb);
    if (m->up_bias) { tr->m_ub = zeros_f32(m->d_hidden); tr->v_ub = zeros_f32(m->d_hidden); }
    tr->fmap = reinterpret_cast<uint2*>(zeros_f32(m->d_hidden * 2));
    tr->touched = reinterpret_cast<uint8_t*>(zeros_f32((m->d_hidden + 3) / 4));
    if (!tr->m_up || !tr->v_up || !tr->m_down || !tr->v_down || !tr->m_db || !tr->v_db || (m->up_bias && (!tr->m_ub || !tr->v_ub)) || !tr->fmap ||
        !tr->touched) {
        mse_sae_trainer_free(tr);
        fail("sae_trainer_create: device allocation failed");
        return nullptr;
    }
    return tr;
}

void mse_sae_trainer_free(mse_sae_trainer* tr) {
    if (!tr) return;
    for (void* p : {(void*)tr->m_up, (void*)tr->v_up, (void*)tr->m_down, (void*)tr->v_down, (void*)tr->m_ub, (void*)tr->v_ub, (void*)tr->m_db,
                    (void*)tr->v_db, (void*)tr->fmap, (void*)tr->touched})
        if (p) (void)hipFree(p);
    delete tr;
}

uint64_t mse_sae_trainer_step_count(const mse_sae_trainer* tr) { return tr ? tr->t : 0; }

int mse_sae_trainer_steps(mse_sae_trainer* tr, const mse_base* b, const uint32_t* ids, size_t batch, size_t n_steps, double* losses_out,
                          size_t* steps_done_out) {
    if (steps_done_out) *steps_done_out = 0;
    if (check_trainer(tr, "sae_trainer_steps")) return -1;
    if (!b || (!ids && n_steps)) return fail("sae_trainer_steps: null base or ids");
    if (b->n && !is_device_pointer(b->dev)) return fail("sae_trainer_steps: the base's rows are not device memory (a wrapped base must wrap a device pointer)");
    if (check_call(tr, b->d, b->device, batch, n_steps, "sae_trainer_steps")) return -1;
    if (n_steps == 0) return 0;
    const size_t total = batch * n_steps;
    for (size_t i = 0; i < total; i++)
        if (ids[i] >= b->n) return fail("sae_trainer_steps: id " + std::to_string(ids[i]) + " at position " + std::to_string(i) + " is not below the " + std::to_string(b->n) + " rows");
    MSE_HIP_TRY(hipSetDevice(tr->device));
    if (tr->ids.ensure(total * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->ids.p, ids, total * 4, hipMemcpyHostToDevice));
    return run_steps(tr, b->dev, tr->ids.as<uint32_t>(), batch, n_steps, losses_out, steps_done_out);
}

int mse_sae_trainer_steps_f16(mse_sae_trainer* tr, const uint16_t* rows_f16, size_t d, size_t batch, size_t n_steps, double* losses_out,
                              size_t* steps_done_out) {
    if (steps_done_out) *steps_done_out = 0;
    if (check_trainer(tr, "sae_trainer_steps_f16")) return -1;
    if (!rows_f16 && n_steps) return fail("sae_trainer_steps_f16: null rows");
    if (check_call(tr, d, tr->device, batch, n_steps, "sae_trainer_steps_f16")) return -1;
    if (n_steps == 0) return 0;
    const size_t total = batch * n_steps;
    MSE_HIP_TRY(hipSetDevice(tr->device));
    if (tr->rows.ensure(total * d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->rows.p, rows_f16, total * d * 2, hipMemcpyHostToDevice));
    return run_steps(tr, tr->rows.as<uint16_t>(), nullptr, batch, n_steps, losses_out, steps_done_out);
}

int mse_sae_trainer_set_skip(mse_sae_trainer* tr, int enable) {
    if (!tr) return fail("sae_trainer_set_skip: null trainer");
    tr->skip = enable != 0;
    return 0;
}

// the moments in the checkpoint's layout: up's as [d_hidden][d_emb], down's as [d_emb][d_hidden]
int mse_sae_trainer_state_read(mse_sae_trainer* tr, uint64_t* t_out, float* m_up, float* v_up, float* m_up_bias_or_null, float* v_up_bias_or_null,
                               float* m_down, float* v_down, float* m_down_bias, float* v_down_bias) {
    if (check_trainer(tr, "sae_trainer_state_read")) return -1;
    mse_sae* m = tr->model;
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t E = m->d_emb, H = m->d_hidden, he = E * H;
    if (t_out) *t_out = tr->t;
    if (m_up) MSE_HIP_TRY(hipMemcpy(m_up, tr->m_up, he * 4, hipMemcpyDeviceToHost));
    if (v_up) MSE_HIP_TRY(hipMemcpy(v_up, tr->v_up, he * 4, hipMemcpyDeviceToHost));
    if (tr->m_ub && m_up_bias_or_null) MSE_HIP_TRY(hipMemcpy(m_up_bias_or_null, tr->m_ub, H * 4, hipMemcpyDeviceToHost));
    if (tr->v_ub && v_up_bias_or_null) MSE_HIP_TRY(hipMemcpy(v_up_bias_or_null, tr->v_ub, H * 4, hipMemcpyDeviceToHost));
    if (m_down_bias) MSE_HIP_TRY(hipMemcpy(m_down_bias, tr->m_db, E * 4, hipMemcpyDeviceToHost));
    if (v_down_bias) MSE_HIP_TRY(hipMemcpy(v_down_bias, tr->v_db, E * 4, hipMemcpyDeviceToHost));
    if (m_down || v_down) {
        DevBuf tmp;
        if (tmp.ensure(he * 4)) return -1;
        for (int which = 0; which < 2; which++) {
            float* out = which ? v_down : m_down;
            if (!out) continue;
            launch_sae_transpose(which ? tr->v_down : tr->m_down, H, E, tmp.as<float>(), nullptr);   // [H][E] -> [E][H]
            MSE_HIP_TRY(hipGetLastError());
            MSE_HIP_TRY(hipStreamSynchronize(nullptr));
            MSE_HIP_TRY(hipMemcpy(out, tmp.p, he * 4, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

int mse_sae_trainer_state_write(mse_sae_trainer* tr, uint64_t t, const float* m_up, const float* v_up, const float* m_up_bias_or_null,
                                const float* v_up_bias_or_null, const float* m_down, const float* v_down, const float* m_down_bias,
                                const float* v_down_bias) {
    if (check_trainer(tr, "sae_trainer_state_write")) return -1;
    mse_sae* m = tr->model;
    if (!m_up || !v_up || !m_down || !v_down || !m_down_bias || !v_down_bias || (m->up_bias && (!m_up_bias_or_null || !v_up_bias_or_null)))
        return fail("sae_trainer_state_write: null moments");
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t E = m->d_emb, H = m->d_hidden, he = E * H;
    MSE_HIP_TRY(hipMemcpy(tr->m_up, m_up, he * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->v_up, v_up, he * 4, hipMemcpyHostToDevice));
    if (tr->m_ub) {
        MSE_HIP_TRY(hipMemcpy(tr->m_ub, m_up_bias_or_null, H * 4, hipMemcpyHostToDevice));
        MSE_HIP_TRY(hipMemcpy(tr->v_ub, v_up_bias_or_null, H * 4, hipMemcpyHostToDevice));
    }
    MSE_HIP_TRY(hipMemcpy(tr->m_db, m_down_bias, E * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->v_db, v_down_bias, E * 4, hipMemcpyHostToDevice));
    DevBuf tmp;
    if (tmp.ensure(he * 4)) return -1;
    for (int which = 0; which < 2; which++) {
        MSE_HIP_TRY(hipMemcpy(tmp.p, which ? v_down : m_down, he * 4, hipMemcpyHostToDevice));
        launch_sae_transpose(tmp.as<float>(), E, H, which ? tr->v_down : tr->m_down, nullptr);   // [E][H] -> [H][E]
        MSE_HIP_TRY(hipGetLastError());
        MSE_HIP_TRY(hipStreamSynchronize(nullptr));
    }
    // a feature counts as touched where any of its moments is not zero (-0 included: only +0 is what the skip's argument needs)
    std::vector<uint8_t> touched(H, 0);
    const uint32_t* bits[2] = {reinterpret_cast<const uint32_t*>(m_up), reinterpret_cast<const uint32_t*>(v_up)};
    for (size_t f = 0; f < H; f++) {
        uint32_t any = 0;
        for (size_t k = 0; k < E; k++) any |= bits[0][f * E + k] | bits[1][f * E + k];
        touched[f] = any ? 1 : 0;
    }
    const uint32_t* dbits[2] = {reinterpret_cast<const uint32_t*>(m_down), reinterpret_cast<const uint32_t*>(v_down)};
    for (size_t k = 0; k < E; k++)
        for (size_t f = 0; f < H; f++)
            if (dbits[0][k * H + f] | dbits[1][k * H + f]) touched[f] = 1;
    MSE_HIP_TRY(hipMemcpy(tr->touched, touched.data(), H, hipMemcpyHostToDevice));
    tr->t = t;
    return 0;
}

int mse_sae_read_weights(mse_sae* m, float* up_or_null, float* up_bias_or_null, float* down_or_null, float* down_bias_or_null) {
    if (!m) return fail("sae_read_weights: null model");
    MSE_HIP_TRY(hipSetDevice(m->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t E = m->d_emb, H = m->d_hidden, he = E * H;
    if (up_or_null) MSE_HIP_TRY(hipMemcpy(up_or_null, m->up, he * 4, hipMemcpyDeviceToHost));
    if (up_bias_or_null && m->up_bias) MSE_HIP_TRY(hipMemcpy(up_bias_or_null, m->up_bias, H * 4, hipMemcpyDeviceToHost));
    if (down_bias_or_null && m->down_bias) MSE_HIP_TRY(hipMemcpy(down_bias_or_null, m->down_bias, E * 4, hipMemcpyDeviceToHost));
    if (down_or_null) {
        DevBuf tmp;
        if (tmp.ensure(he * 4)) return -1;
        launch_sae_transpose(m->downT, H, E, tmp.as<float>(), nullptr);   // [H][E] -> [E][H]
        MSE_HIP_TRY(hipGetLastError());
        MSE_HIP_TRY(hipStreamSynchronize(nullptr));
        MSE_HIP_TRY(hipMemcpy(down_or_null, tmp.p, he * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

int mse_sae_trainer_timing(int enable, double* out_or_null) {
    std::lock_guard<std::mutex> g(g_tm_mu);
    if (out_or_null)
        for (int i = 0; i < 4; i++) out_or_null[i] = g_tm[i];
    g_tm_on = enable != 0;
    if (enable == 2) g_tm[0] = g_tm[1] = g_tm[2] = g_tm[3] = 0.0;
    return 0;
}

}  // extern "C"
