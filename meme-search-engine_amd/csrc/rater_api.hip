// C ABI of the ensemble rater (kernels: rater.hip): the model handle `mse_rater` in the wide layout, its trainer `mse_rater_trainer`
// (meme-rater/train.py:63-71 on the device, in place), the member-score table `mse_member_scores` and the disagreement of candidate
// pairs over it (active_learning.py:44-56).  A training call of many steps is queued whole on the null stream -- the gate is a device
// flag -- and returns with the stream drained.
#include "../../include/mse.h"
#include "rater.h"
#include <cmath>
#include <new>
#include <unordered_map>

using namespace mse;

struct mse_rater {
    uint64_t uid = 0;            // how a trainer recognises its model among the live ones (an address can be reused)
    int device = 0, n_cu = 256;
    size_t E = 0, M = 0, C = 0;
    float *up = nullptr, *bias = nullptr, *down = nullptr;   // device: [M E][E], [M E], [C][M E]
    std::mutex mu;               // guards the scratch below and -- against a training call -- the weights
    DevBuf h, ids, rows;
};

struct mse_rater_trainer {
    mse_rater* model = nullptr;
    uint64_t model_uid = 0;
    int device = 0;
    double lr = 0, beta1 = 0, beta2 = 0, eps = 0, wd = 0;
    uint64_t t = 0;              // completed steps since the moments were zero (or since state_write)
    size_t last_batch = 0;       // of the last completed step: what `s` holds
    float *m_up = nullptr, *v_up = nullptr, *m_bias = nullptr, *v_bias = nullptr, *m_down = nullptr, *v_down = nullptr;
    DevBuf u, h, du, s, g, tab, targets, rows, losses, hyper, ctl;
};

struct mse_member_scores {
    int device = 0;
    size_t n = 0, M = 0, C = 0;
    float* s = nullptr;          // device [n][M][C]
    std::mutex mu;
    DevBuf a, b, out;
};

namespace {

std::mutex g_live_mu;
std::unordered_map<const mse_rater*, uint64_t> g_live;
uint64_t g_next_uid = 1;

std::mutex g_tm_mu;
bool g_tm_on = false;
double g_tm[4] = {0.0, 0.0, 0.0, 0.0};   // forward, backward, update milliseconds and the steps they cover

constexpr size_t SCORE_CHUNK_BYTES = (size_t)256 << 20;   // of hidden activations one launch of the member scores may hold

bool rater_alive(const mse_rater* r, uint64_t uid) {
    std::lock_guard<std::mutex> g(g_live_mu);
    auto it = g_live.find(r);
    return it != g_live.end() && it->second == uid;
}

bool is_device_pointer(const void* p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

float* device_f32(const float* host_or_null, size_t count) {
    float* p = nullptr;
    const size_t bytes = std::max<size_t>(count * 4, 256);
    if (hipMalloc((void**)&p, bytes) != hipSuccess) return nullptr;
    const hipError_t e = host_or_null ? hipMemcpy(p, host_or_null, count * 4, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
    if (e != hipSuccess) { (void)hipFree(p); return nullptr; }
    return p;
}

int check_trainer(const mse_rater_trainer* tr, const char* who) {
    if (!tr) return fail(std::string(who) + ": null trainer");
    if (!rater_alive(tr->model, tr->model_uid)) return fail(std::string(who) + ": the trainer's rater has been freed");
    return 0;
}

int check_call(const mse_rater_trainer* tr, size_t d, int device, size_t batch, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    const mse_rater* m = tr->model;
    if (m->E != d) return fail(who + "the rater's d_emb is " + std::to_string(m->E) + " but the rows have " + std::to_string(d) + " components");
    if (m->device != device) return fail(who + "the rater lives on device " + std::to_string(m->device) + " and the rows on device " + std::to_string(device));
    if (batch == 0) return fail(who + "an empty batch");
    if (batch > RATER_MAX_BATCH) return fail(who + "a batch of " + std::to_string(batch) + " pairs (at most " + std::to_string(RATER_MAX_BATCH) + ")");
    return 0;
}

// n_steps steps of `batch` pairs per member over the device rows: step s, member m, slot r is row tab[(s M + m) 2 batch + r]; the table
// and the targets [n_steps][M][batch][C] are on the device already
int run_steps(mse_rater_trainer* tr, const uint16_t* rows, size_t batch, size_t n_steps, double* losses_out, size_t* steps_done_out) {
    mse_rater* m = tr->model;
    const size_t B = batch, R = 2 * B, E = m->E, M = m->M, Cc = m->C, slots = M * R * E;
    if (tr->u.ensure(slots * 4) || tr->h.ensure(slots * 4) || tr->du.ensure(slots * 4) || tr->s.ensure(M * R * Cc * 4) ||
        tr->g.ensure(M * B * Cc * 4) || tr->losses.ensure(n_steps * 8) || tr->hyper.ensure(n_steps * sizeof(SaeAdamStep)) || tr->ctl.ensure(256))
        return -1;
    std::vector<SaeAdamStep> hyper(n_steps);
    for (size_t s = 0; s < n_steps; s++) {
        const double t = (double)(tr->t + s + 1);
        hyper[s].decay = (float)(1.0 - tr->lr * tr->wd);
        hyper[s].step_size = (float)(tr->lr / (1.0 - std::pow(tr->beta1, t)));
        hyper[s].bc2_sqrt = (float)std::sqrt(1.0 - std::pow(tr->beta2, t));
    }
    MSE_HIP_TRY(hipMemcpy(tr->hyper.p, hyper.data(), n_steps * sizeof(SaeAdamStep), hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemsetAsync(tr->ctl.p, 0, sizeof(RaterCtl), nullptr));
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
    RaterStep st{};
    st.ctl = tr->ctl.as<RaterCtl>();
    st.adam = SaeAdam{(float)tr->beta1, (float)tr->beta2, (float)tr->eps};
    st.E = (int)E; st.M = (int)M; st.C = (int)Cc; st.B = (int)B;
    st.rows = rows;
    st.inv_n = (float)(1.0 / (double)(M * B * Cc));
    st.u = tr->u.as<float>(); st.h = tr->h.as<float>(); st.du = tr->du.as<float>(); st.s = tr->s.as<float>(); st.g = tr->g.as<float>();
    st.up = m->up; st.m_up = tr->m_up; st.v_up = tr->v_up; st.bias = m->bias; st.m_bias = tr->m_bias; st.v_bias = tr->v_bias;
    st.down = m->down; st.m_down = tr->m_down; st.v_down = tr->v_down;
    st.n_cu = m->n_cu;
    const uint32_t* const stop = &st.ctl->stop;
    auto queue = [&]() -> int {
        for (size_t s = 0; s < n_steps; s++) {
            st.hyper = tr->hyper.as<SaeAdamStep>() + s;
            st.loss = tr->losses.as<double>() + s;
            st.tab = tr->tab.as<uint32_t>() + s * M * R;
            st.targets = tr->targets.as<float>() + s * M * B * Cc;
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s], nullptr));
            launch_rater_forward(rows, (int)E, (int)M, st.tab, R, 0, R, m->up, m->bias, st.u, st.h, stop, nullptr);
            launch_rater_scores(st.h, m->down, (int)E, (int)M, (int)Cc, R, st.s, R * Cc, Cc, stop, nullptr);
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s + 1], nullptr));
            launch_rater_backward(st, nullptr);
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s + 2], nullptr));
            launch_rater_update(st, nullptr);
            if (tm) MSE_HIP_TRY(hipEventRecord(ev[4 * s + 3], nullptr));
            MSE_HIP_TRY(hipGetLastError());
        }
        return 0;
    };
    const int rc = queue();
    if (hipStreamSynchronize(nullptr) != hipSuccess && rc == 0) return fail("rater_trainer_steps: the device reported an error");
    RaterCtl ctl{};
    MSE_HIP_TRY(hipMemcpy(&ctl, tr->ctl.p, sizeof ctl, hipMemcpyDeviceToHost));
    const size_t done = std::min<size_t>(ctl.steps_done, n_steps);
    tr->t += done;
    tr->last_batch = done == n_steps ? B : 0;   // after a refusal `s` holds the refused step's scores
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

// the checks and uploads both training entry points share: every id below n_rows, the slot table and the targets onto the device
int stage_steps(mse_rater_trainer* tr, const uint32_t* pair_ids, const float* targets, size_t n_rows, size_t batch, size_t n_steps, const char* who) {
    const mse_rater* m = tr->model;
    if (n_steps > 0xFFFFFFFFull / (m->M * 2 * batch * std::max<size_t>(m->C, 2))) return fail(std::string(who) + ": too many steps for one call");
    const size_t n_ids = n_steps * m->M * batch * 2, n_t = n_steps * m->M * batch * m->C;
    for (size_t i = 0; i < n_ids; i++)
        if (pair_ids[i] >= n_rows)
            return fail(std::string(who) + ": id " + std::to_string(pair_ids[i]) + " at position " + std::to_string(i) + " is not below the " + std::to_string(n_rows) + " rows");
    if (tr->tab.ensure(n_ids * 4) || tr->targets.ensure(n_t * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->tab.p, pair_ids, n_ids * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->targets.p, targets, n_t * 4, hipMemcpyHostToDevice));
    return 0;
}

// the body of mse_member_scores_from_base / _from_f16 over rows [n_rows][d] on the rater's device, under the rater's lock, which the
// caller holds; returns drained
mse_member_scores* scores_from_rows(mse_rater* m, const uint16_t* rows_dev, size_t n_rows, size_t d, int device, const uint32_t* ids_or_null,
                                    size_t first, size_t n, const char* who_c) {
    const std::string who = std::string(who_c) + ": ";
    if (m->E != d) { fail(who + "the rater's d_emb is " + std::to_string(m->E) + " but the rows have " + std::to_string(d) + " components"); return nullptr; }
    if (m->device != device) { fail(who + "the rater lives on device " + std::to_string(m->device) + " and the rows on device " + std::to_string(device)); return nullptr; }
    if (!ids_or_null && (first > n_rows || n > n_rows - first)) { fail(who + "rows " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(n) + " are not within the " + std::to_string(n_rows) + " rows"); return nullptr; }
    if (n > 0xFFFFFFFFull) { fail(who + "too many rows for one call"); return nullptr; }
    if (ids_or_null)
        for (size_t i = 0; i < n; i++)
            if (ids_or_null[i] >= n_rows) { fail(who + "id " + std::to_string(ids_or_null[i]) + " at position " + std::to_string(i) + " is not below the " + std::to_string(n_rows) + " rows"); return nullptr; }
    if (ids_or_null && n) {
        if (m->ids.ensure(n * 4)) return nullptr;
        MSE_HIP_TRY_PTR(hipMemcpy(m->ids.p, ids_or_null, n * 4, hipMemcpyHostToDevice));
    }
    mse_member_scores* s = new (std::nothrow) mse_member_scores();
    if (!s) { fail("out of host memory"); return nullptr; }
    s->device = device; s->n = n; s->M = m->M; s->C = m->C;
    if (hipMalloc((void**)&s->s, std::max<size_t>(n * m->M * m->C * 4, 256)) != hipSuccess) {
        delete s;
        fail(who + "device allocation failed");
        return nullptr;
    }
    // rows per launch: whole forward tiles whose activations [M][rows][E] fit the budget
    const size_t per_row = m->M * m->E * 4;
    const size_t chunk = std::max<size_t>(1, SCORE_CHUNK_BYTES / per_row / 128) * 128;
    if (n && m->h.ensure(std::min(chunk, n) * per_row)) { mse_member_scores_free(s); return nullptr; }
    for (size_t at = 0; at < n; at += chunk) {
        const size_t cn = std::min(chunk, n - at);
        launch_rater_forward(rows_dev, (int)m->E, (int)m->M, ids_or_null ? m->ids.as<uint32_t>() + at : nullptr, 0, first + at, cn, m->up, m->bias,
                             nullptr, m->h.as<float>(), nullptr, nullptr);
        launch_rater_scores(m->h.as<float>(), m->down, (int)m->E, (int)m->M, (int)m->C, cn, s->s + at * m->M * m->C, m->C, m->M * m->C, nullptr, nullptr);
    }
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(nullptr);
    if (e1 != hipSuccess || e2 != hipSuccess) {
        mse_member_scores_free(s);
        fail(who + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return nullptr;
    }
    return s;
}

}  // namespace

extern "C" {

mse_rater* mse_rater_create(const float* up, const float* bias, const float* down, size_t d_emb, size_t n_members, size_t out_channels) {
    if (!up || !bias || !down) { fail("rater_create: null weights"); return nullptr; }
    if (d_emb < 1 || d_emb > ((size_t)1 << 20)) { fail("rater_create: d_emb must be in 1 .. 2^20"); return nullptr; }
    if (n_members < 1 || n_members > RATER_MAX_MEMBERS) { fail("rater_create: " + std::to_string(n_members) + " members (1 .. " + std::to_string(RATER_MAX_MEMBERS) + ")"); return nullptr; }
    if (out_channels < 1 || out_channels > RATER_MAX_CHANNELS) { fail("rater_create: " + std::to_string(out_channels) + " output channels (1 .. " + std::to_string(RATER_MAX_CHANNELS) + ")"); return nullptr; }
    int device = 0;
    MSE_HIP_TRY_PTR(hipGetDevice(&device));
    mse_rater* m = new (std::nothrow) mse_rater();
    if (!m) { fail("out of host memory"); return nullptr; }
    m->device = device;
    m->n_cu = device_cu_count();
    m->E = d_emb; m->M = n_members; m->C = out_channels;
    const size_t H = n_members * d_emb;
    m->up = device_f32(up, H * d_emb);
    m->bias = device_f32(bias, H);
    m->down = device_f32(down, out_channels * H);
    if (!m->up || !m->bias || !m->down) {
        mse_rater_free(m);
        fail("rater_create: device allocation failed");
        return nullptr;
    }
    std::lock_guard<std::mutex> g(g_live_mu);
    m->uid = g_next_uid++;
    g_live[m] = m->uid;
    return m;
}

void mse_rater_free(mse_rater* m) {
    if (!m) return;
    { std::lock_guard<std::mutex> g(g_live_mu); g_live.erase(m); }
    for (void* p : {(void*)m->up, (void*)m->bias, (void*)m->down})
        if (p) (void)hipFree(p);
    delete m;
}

int mse_rater_read_weights(mse_rater* m, float* up_or_null, float* bias_or_null, float* down_or_null) {
    if (!m) return fail("rater_read_weights: null rater");
    MSE_HIP_TRY(hipSetDevice(m->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t H = m->M * m->E;
    if (up_or_null) MSE_HIP_TRY(hipMemcpy(up_or_null, m->up, H * m->E * 4, hipMemcpyDeviceToHost));
    if (bias_or_null) MSE_HIP_TRY(hipMemcpy(bias_or_null, m->bias, H * 4, hipMemcpyDeviceToHost));
    if (down_or_null) MSE_HIP_TRY(hipMemcpy(down_or_null, m->down, m->C * H * 4, hipMemcpyDeviceToHost));
    return 0;
}

mse_rater_trainer* mse_rater_trainer_create(mse_rater* m, double lr, double beta1, double beta2, double eps, double weight_decay) {
    if (!m) { fail("rater_trainer_create: null rater"); return nullptr; }
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(lr >= 0.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) ||
        !std::isfinite(lr) || !std::isfinite(eps) || !std::isfinite(weight_decay)) {
        fail("rater_trainer_create: invalid AdamW parameters");
        return nullptr;
    }
    MSE_HIP_TRY_PTR(hipSetDevice(m->device));
    mse_rater_trainer* tr = new (std::nothrow) mse_rater_trainer();
    if (!tr) { fail("out of host memory"); return nullptr; }
    tr->model = m; tr->model_uid = m->uid; tr->device = m->device;
    tr->lr = lr; tr->beta1 = beta1; tr->beta2 = beta2; tr->eps = eps; tr->wd = weight_decay;
    const size_t H = m->M * m->E;
    tr->m_up = device_f32(nullptr, H * m->E); tr->v_up = device_f32(nullptr, H * m->E);
    tr->m_bias = device_f32(nullptr, H); tr->v_bias = device_f32(nullptr, H);
    tr->m_down = device_f32(nullptr, m->C * H); tr->v_down = device_f32(nullptr, m->C * H);
    if (!tr->m_up || !tr->v_up || !tr->m_bias || !tr->v_bias || !tr->m_down || !tr->v_down) {
        mse_rater_trainer_free(tr);
        fail("rater_trainer_create: device allocation failed");
        return nullptr;
    }
    return tr;
}

void mse_rater_trainer_free(mse_rater_trainer* tr) {
    if (!tr) return;
    for (void* p : {(void*)tr->m_up, (void*)tr->v_up, (void*)tr->m_bias, (void*)tr->v_bias, (void*)tr->m_down, (void*)tr->v_down})
        if (p) (void)hipFree(p);
    delete tr;
}

uint64_t mse_rater_trainer_step_count(const mse_rater_trainer* tr) { return tr ? tr->t : 0; }

int mse_rater_trainer_steps(mse_rater_trainer* tr, const mse_base* b, const uint32_t* pair_ids, const float* targets, size_t batch, size_t n_steps,
                            double* losses_out, size_t* steps_done_out) {
    if (steps_done_out) *steps_done_out = 0;
    if (check_trainer(tr, "rater_trainer_steps")) return -1;
    if (!b || ((!pair_ids || !targets) && n_steps)) return fail("rater_trainer_steps: null base, ids or targets");
    if (b->n && !is_device_pointer(b->dev)) return fail("rater_trainer_steps: the base's rows are not device memory (a wrapped base must wrap a device pointer)");
    if (check_call(tr, b->d, b->device, batch, "rater_trainer_steps")) return -1;
    if (n_steps == 0) return 0;
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(tr->model->mu);
    if (stage_steps(tr, pair_ids, targets, b->n, batch, n_steps, "rater_trainer_steps")) return -1;
    return run_steps(tr, b->dev, batch, n_steps, losses_out, steps_done_out);
}

int mse_rater_trainer_steps_f16(mse_rater_trainer* tr, const uint16_t* rows_f16, size_t n_rows, size_t d, const uint32_t* pair_idx, const float* targets,
                                size_t batch, size_t n_steps, double* losses_out, size_t* steps_done_out) {
    if (steps_done_out) *steps_done_out = 0;
    if (check_trainer(tr, "rater_trainer_steps_f16")) return -1;
    if ((!rows_f16 || !pair_idx || !targets) && n_steps) return fail("rater_trainer_steps_f16: null rows, indices or targets");
    if (check_call(tr, d, tr->device, batch, "rater_trainer_steps_f16")) return -1;
    if (n_steps == 0) return 0;
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(tr->model->mu);
    if (stage_steps(tr, pair_idx, targets, n_rows, batch, n_steps, "rater_trainer_steps_f16")) return -1;
    if (tr->rows.ensure(n_rows * d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->rows.p, rows_f16, n_rows * d * 2, hipMemcpyHostToDevice));
    return run_steps(tr, tr->rows.as<uint16_t>(), batch, n_steps, losses_out, steps_done_out);
}

int mse_rater_trainer_state_read(mse_rater_trainer* tr, uint64_t* t_out, float* m_up, float* v_up, float* m_bias, float* v_bias, float* m_down,
                                 float* v_down) {
    if (check_trainer(tr, "rater_trainer_state_read")) return -1;
    mse_rater* m = tr->model;
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t H = m->M * m->E;
    if (t_out) *t_out = tr->t;
    if (m_up) MSE_HIP_TRY(hipMemcpy(m_up, tr->m_up, H * m->E * 4, hipMemcpyDeviceToHost));
    if (v_up) MSE_HIP_TRY(hipMemcpy(v_up, tr->v_up, H * m->E * 4, hipMemcpyDeviceToHost));
    if (m_bias) MSE_HIP_TRY(hipMemcpy(m_bias, tr->m_bias, H * 4, hipMemcpyDeviceToHost));
    if (v_bias) MSE_HIP_TRY(hipMemcpy(v_bias, tr->v_bias, H * 4, hipMemcpyDeviceToHost));
    if (m_down) MSE_HIP_TRY(hipMemcpy(m_down, tr->m_down, m->C * H * 4, hipMemcpyDeviceToHost));
    if (v_down) MSE_HIP_TRY(hipMemcpy(v_down, tr->v_down, m->C * H * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_rater_trainer_state_write(mse_rater_trainer* tr, uint64_t t, const float* m_up, const float* v_up, const float* m_bias, const float* v_bias,
                                  const float* m_down, const float* v_down) {
    if (check_trainer(tr, "rater_trainer_state_write")) return -1;
    if (!m_up || !v_up || !m_bias || !v_bias || !m_down || !v_down) return fail("rater_trainer_state_write: null moments");
    mse_rater* m = tr->model;
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(m->mu);
    const size_t H = m->M * m->E;
    MSE_HIP_TRY(hipMemcpy(tr->m_up, m_up, H * m->E * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->v_up, v_up, H * m->E * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->m_bias, m_bias, H * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->v_bias, v_bias, H * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->m_down, m_down, m->C * H * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->v_down, v_down, m->C * H * 4, hipMemcpyHostToDevice));
    tr->t = t;
    return 0;
}

int mse_rater_trainer_last_scores(mse_rater_trainer* tr, float* out, size_t* batch_out) {
    if (check_trainer(tr, "rater_trainer_last_scores")) return -1;
    if (batch_out) *batch_out = tr->last_batch;
    if (!tr->last_batch) return fail("rater_trainer_last_scores: no completed step to read");
    MSE_HIP_TRY(hipSetDevice(tr->device));
    std::lock_guard<std::mutex> g(tr->model->mu);
    if (out) MSE_HIP_TRY(hipMemcpy(out, tr->s.p, tr->model->M * 2 * tr->last_batch * tr->model->C * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_rater_trainer_timing(int enable, double* out_or_null) {
    std::lock_guard<std::mutex> g(g_tm_mu);
    if (out_or_null)
        for (int i = 0; i < 4; i++) out_or_null[i] = g_tm[i];
    g_tm_on = enable != 0;
    if (enable == 2) g_tm[0] = g_tm[1] = g_tm[2] = g_tm[3] = 0.0;
    return 0;
}

mse_member_scores* mse_member_scores_from_base(mse_rater* m, const mse_base* b, const uint32_t* ids_or_null, size_t first, size_t n) {
    if (!m || !b) { fail("member_scores_from_base: null rater or base"); return nullptr; }
    if (b->n && !is_device_pointer(b->dev)) { fail("member_scores_from_base: the base's rows are not device memory (a wrapped base must wrap a device pointer)"); return nullptr; }
    MSE_HIP_TRY_PTR(hipSetDevice(m->device));
    std::lock_guard<std::mutex> g(m->mu);
    return scores_from_rows(m, b->dev, b->n, b->d, b->device, ids_or_null, first, n, "member_scores_from_base");
}

mse_member_scores* mse_member_scores_from_f16(mse_rater* m, const uint16_t* rows_f16, size_t n_rows, size_t d, const uint32_t* ids_or_null, size_t first,
                                              size_t n) {
    if (!m || (!rows_f16 && n_rows)) { fail("member_scores_from_f16: null rater or rows"); return nullptr; }
    MSE_HIP_TRY_PTR(hipSetDevice(m->device));
    std::lock_guard<std::mutex> g(m->mu);
    if (m->rows.ensure(std::max<size_t>(n_rows * d * 2, 16))) return nullptr;
    if (n_rows) MSE_HIP_TRY_PTR(hipMemcpy(m->rows.p, rows_f16, n_rows * d * 2, hipMemcpyHostToDevice));
    return scores_from_rows(m, m->rows.as<uint16_t>(), n_rows, d, m->device, ids_or_null, first, n, "member_scores_from_f16");
}

void mse_member_scores_free(mse_member_scores* s) {
    if (!s) return;
    if (s->s) (void)hipFree(s->s);
    delete s;
}

size_t mse_member_scores_len(const mse_member_scores* s) { return s ? s->n : 0; }

int mse_member_scores_read(const mse_member_scores* s, float* out) {
    if (!s || !out) return fail("member_scores_read: null table or output");
    MSE_HIP_TRY(hipSetDevice(s->device));
    if (s->n) MSE_HIP_TRY(hipMemcpy(out, s->s, s->n * s->M * s->C * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_member_scores_pair_variance(mse_member_scores* s, const uint32_t* a_idx, const uint32_t* b_idx, size_t n_pairs, float* out) {
    if (!s) return fail("member_scores_pair_variance: null table");
    if (s->M < 2) return fail("member_scores_pair_variance: the variance over one member is undefined (torch.var's correction divides by M - 1)");
    if (n_pairs == 0) return 0;
    if (!a_idx || !b_idx || !out) return fail("member_scores_pair_variance: null indices or output");
    for (size_t i = 0; i < n_pairs; i++)
        if (a_idx[i] >= s->n || b_idx[i] >= s->n)
            return fail("member_scores_pair_variance: pair " + std::to_string(i) + " names a row that is not below the table's " + std::to_string(s->n));
    MSE_HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> g(s->mu);
    if (s->a.ensure(n_pairs * 4) || s->b.ensure(n_pairs * 4) || s->out.ensure(n_pairs * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(s->a.p, a_idx, n_pairs * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(s->b.p, b_idx, n_pairs * 4, hipMemcpyHostToDevice));
    launch_rater_pair_variance(s->s, (int)s->M, (int)s->C, s->a.as<uint32_t>(), s->b.as<uint32_t>(), n_pairs, s->out.as<float>(), nullptr);
    MSE_HIP_TRY(hipGetLastError());
    MSE_HIP_TRY(hipStreamSynchronize(nullptr));
    MSE_HIP_TRY(hipMemcpy(out, s->out.p, n_pairs * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
