// C ABI (include/mse.h): the codec trainer -- diskann/aopq_train.py:33-85 on the device -- and the test hooks of its two kernels.
// The kernels are in pq_train.hip; the rotation and the assignment are pq.hip's.  DESIGN.md 3.20 has the definitions.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace mse;

struct mse_pq_trainer {
    size_t d = 0, dpc = 0, n_chunks = 0, n_cells = 0;
    int device = 0;
    size_t n = 0;                  // sample rows
    bool from_base = false;        // the unrotated sample is x16 (f16 rows gathered from a base), else x32
    bool have_T = false, have_cent = false, have_C0 = false;
    size_t chunk_rows = 262144;    // rows per pass of the residual GEMM: G is a scratch of chunk_rows x d floats (1.2 GB at d = 1152)
    DevBuf x16, x32, xr, wide;     // the sample, its rotation X', the widening scratch of the re-rotation
    DevBuf codes, cent, T, C0, Cm, tmp_a, tmp_b;
    DevBuf m, v, grad;             // Adam moments and the last step's gradient, [n_cells][d]
    bool have_grad = false;
    uint64_t t = 0;                // Adam step count
    DevBuf G, lpart, lrow;
    DevBuf sums, counts, sigma, M, loss, ids, zeros;
    DevBuf slots;                  // u32 max_bits[S] | i32 E[S] | u32 err | u64 empty | i64 loss sum; slot 0: X', 1: l_row, 2 + c: G of row chunk c
    size_t n_slots = 0;
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
};

namespace {

size_t row_chunks(const mse_pq_trainer* tr) { return tr->n ? (tr->n + tr->chunk_rows - 1) / tr->chunk_rows : 1; }
uint32_t* slot_max(mse_pq_trainer* tr, size_t s) { return tr->slots.as<uint32_t>() + s; }
int* slot_E(mse_pq_trainer* tr, size_t s) { return tr->slots.as<int>() + tr->n_slots + s; }
char* slot_tail(mse_pq_trainer* tr) { return tr->slots.as<char>() + ((tr->n_slots * 8 + 15) & ~(size_t)15); }
uint32_t* slot_err(mse_pq_trainer* tr) { return reinterpret_cast<uint32_t*>(slot_tail(tr)); }
unsigned long long* slot_empty(mse_pq_trainer* tr) { return reinterpret_cast<unsigned long long*>(slot_tail(tr) + 8); }
long long* slot_loss_sum(mse_pq_trainer* tr) { return reinterpret_cast<long long*>(slot_tail(tr) + 16); }

int ensure_slots(mse_pq_trainer* tr) {
    const size_t want = 2 + row_chunks(tr);
    if (tr->slots.p && tr->n_slots >= want) return 0;
    tr->n_slots = want;
    const size_t bytes = ((want * 8 + 15) & ~(size_t)15) + 32;
    if (tr->slots.ensure(bytes)) return -1;
    MSE_HIP_TRY(hipMemset(tr->slots.p, 0, bytes));
    return 0;
}

// a pending non-finite value (bit 0 of the device error word) becomes the call's error; the word is cleared
int take_error(mse_pq_trainer* tr, const char* who) {
    uint32_t err = 0;
    MSE_HIP_TRY(hipMemcpy(&err, slot_err(tr), 4, hipMemcpyDeviceToHost));
    if (err) {
        MSE_HIP_TRY(hipMemset(slot_err(tr), 0, 4));
        return fail(std::string(who) + ": a non-finite value reached the order-free sum");
    }
    return 0;
}

int scope_check(mse_pq_trainer* tr, const char* who) {
    if (!tr) return fail(std::string(who) + ": null trainer");
    return 0;
}

// X' = rows of the ORIGINAL sample through launch_pq_transform, 65536 rows at a time, and the exponent of its order-free sums
int rerotate(mse_pq_trainer* tr) {
    if (!tr->n || !tr->have_T) return 0;
    const size_t d = tr->d, step = 65536;
    if (tr->xr.ensure(tr->n * d * 4)) return -1;
    if (tr->from_base && tr->wide.ensure(std::min(step, tr->n) * d * 4)) return -1;
    for (size_t r0 = 0; r0 < tr->n; r0 += step) {
        const size_t mrows = std::min(step, tr->n - r0);
        const float* src = tr->x32.as<float>() + r0 * d;
        if (tr->from_base) {
            if (launch_f16_to_f32(tr->x16.as<uint16_t>() + r0 * d, mrows * d, tr->wide.as<float>(), nullptr)) return -1;
            src = tr->wide.as<float>();
        }
        if (launch_pq_transform(tr->T.as<float>(), (int)d, src, mrows, tr->xr.as<float>() + r0 * d, nullptr)) return -1;
    }
    if (ensure_slots(tr)) return -1;
    if (launch_abs_max(tr->xr.as<float>(), tr->n * d, slot_max(tr, 0), nullptr) ||
        launch_fixed_exponent(slot_max(tr, 0), tr->n, slot_E(tr, 0), slot_err(tr), nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    return take_error(tr, "pq_trainer: the rotated sample");
}

// C = T C0 T^T as two passes of the rotation kernel: W = rows of C0 rotated, C = rows of W^T rotated
int rotate_moment(mse_pq_trainer* tr) {
    if (!tr->have_T || !tr->have_C0) return 0;
    const size_t d = tr->d, bytes = d * d * 4;
    if (tr->tmp_a.ensure(bytes) || tr->tmp_b.ensure(bytes) || tr->Cm.ensure(bytes)) return -1;
    if (launch_pq_transform(tr->T.as<float>(), (int)d, tr->C0.as<float>(), d, tr->tmp_a.as<float>(), nullptr) ||
        launch_transpose_f32(tr->tmp_a.as<float>(), (int)d, tr->tmp_b.as<float>(), nullptr) ||
        launch_pq_transform(tr->T.as<float>(), (int)d, tr->tmp_b.as<float>(), d, tr->Cm.as<float>(), nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int need_state(mse_pq_trainer* tr, const char* who, bool moment) {
    if (!tr->n) return fail(std::string(who) + ": no sample set");
    if (!tr->have_T) return fail(std::string(who) + ": no transform set");
    if (!tr->have_cent) return fail(std::string(who) + ": no centroids set");
    if (moment && !tr->have_C0) return fail(std::string(who) + ": no query moment set (mse_pq_trainer_set_query_moment)");
    return 0;
}

int assign(mse_pq_trainer* tr) {
    if (tr->codes.ensure(tr->n * tr->n_chunks)) return -1;
    return launch_pq_quantize(tr->cent.as<float>(), (int)tr->n_cells, (int)tr->d, (int)tr->dpc, tr->xr.as<float>(), tr->n, tr->codes.as<uint8_t>(), nullptr);
}

struct StepEvents {
    std::vector<hipEvent_t> ev;
    hipEvent_t mark() {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        (void)hipEventRecord(e, nullptr);
        ev.push_back(e);
        return e;
    }
    ~StepEvents() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
float span(hipEvent_t a, hipEvent_t b) {
    float msv = 0.0f;
    if (!a || !b || hipEventElapsedTime(&msv, a, b) != hipSuccess) { (void)hipGetLastError(); return 0.0f; }
    return msv;
}

// assignment, G = R C per row chunk (sums of its 18-column blocks by code when with_grad), l_row, and the loss into loss_out (device).
// timed: the spans of the step go to tr->ms[0..2]
int forward(mse_pq_trainer* tr, bool with_grad, double* loss_out, StepEvents* timed) {
    const size_t d = tr->d, n = tr->n, chunks = row_chunks(tr), per = tr->n_chunks * tr->n_cells * tr->dpc;
    const int parts = residual_gemm_parts((int)d);
    if (ensure_slots(tr)) return -1;
    if (tr->lpart.ensure(std::min(n, tr->chunk_rows) * parts * 4) || tr->lrow.ensure(n * 4)) return -1;
    if (with_grad && (tr->G.ensure(std::min(n, tr->chunk_rows) * d * 4) || tr->sums.ensure(chunks * per * 8))) return -1;
    hipEvent_t a0 = timed ? timed->mark() : nullptr;
    if (assign(tr)) return -1;
    hipEvent_t a1 = timed ? timed->mark() : nullptr;
    if (with_grad) MSE_HIP_TRY(hipMemsetAsync(tr->sums.p, 0, chunks * per * 8, nullptr));
    std::vector<hipEvent_t> marks;
    for (size_t c = 0; c < chunks; c++) {
        const size_t r0 = c * tr->chunk_rows, mrows = std::min(tr->chunk_rows, n - r0);
        if (timed) marks.push_back(timed->mark());
        if (launch_residual_gemm(tr->xr.as<float>() + r0 * d, tr->codes.as<uint8_t>() + r0 * tr->n_chunks, tr->cent.as<float>(), tr->Cm.as<float>(), mrows,
                                 (int)d, (int)tr->dpc, with_grad ? tr->G.as<float>() : nullptr, tr->lpart.as<float>(), tr->lrow.as<float>() + r0, nullptr)) return -1;
        if (timed) marks.push_back(timed->mark());
        if (with_grad) {
            if (launch_abs_max(tr->G.as<float>(), mrows * d, slot_max(tr, 2 + c), nullptr) ||
                launch_fixed_exponent(slot_max(tr, 2 + c), mrows, slot_E(tr, 2 + c), slot_err(tr), nullptr)) return -1;
            AccumulateArgs a;
            a.v = tr->G.as<float>(); a.n = mrows; a.w = (int)tr->dpc; a.v_stride = d; a.v_step = (int)tr->dpc;
            a.code = tr->codes.as<uint8_t>() + r0 * tr->n_chunks; a.code_stride = tr->n_chunks; a.code_step = 1;
            a.n_cells = (int)tr->n_cells; a.n_slices = (int)tr->n_chunks; a.E = slot_E(tr, 2 + c);
            a.sums = tr->sums.as<long long>() + c * per; a.sums_step = tr->n_cells * tr->dpc;
            if (launch_accumulate_by_code(a, nullptr)) return -1;
        }
        if (timed) marks.push_back(timed->mark());
    }
    // L = (order-free sum of l_row over the rows) / n
    MSE_HIP_TRY(hipMemsetAsync(slot_loss_sum(tr), 0, 8, nullptr));
    if (launch_abs_max(tr->lrow.as<float>(), n, slot_max(tr, 1), nullptr) ||
        launch_fixed_exponent(slot_max(tr, 1), n, slot_E(tr, 1), slot_err(tr), nullptr)) return -1;
    if (tr->zeros.ensure(n)) return -1;      // one cell: every row has code 0
    MSE_HIP_TRY(hipMemsetAsync(tr->zeros.p, 0, n, nullptr));
    AccumulateArgs l;
    l.v = tr->lrow.as<float>(); l.n = n; l.w = 1; l.v_stride = 1; l.code = tr->zeros.as<uint8_t>(); l.code_stride = 1;
    l.n_cells = 1; l.E = slot_E(tr, 1); l.sums = slot_loss_sum(tr);
    if (launch_accumulate_by_code(l, nullptr) || launch_loss_finish(slot_loss_sum(tr), slot_E(tr, 1), n, loss_out, nullptr)) return -1;
    if (timed) {
        MSE_HIP_TRY(hipDeviceSynchronize());
        tr->ms[0] = span(a0, a1);
        tr->ms[1] = tr->ms[2] = 0.0f;
        for (size_t c = 0; c + 2 < marks.size(); c += 3) {
            tr->ms[1] += span(marks[c], marks[c + 1]);
            tr->ms[2] += span(marks[c + 1], marks[c + 2]);
        }
    }
    return 0;
}

bool shape_ok(size_t n_dims, size_t dpc, size_t n_centroids) {
    if (n_centroids == 0 || n_centroids > 256) { fail("at most 256 centroids (vector.rs:337)"); return false; }
    if (n_dims == 0 || dpc == 0 || n_dims % dpc != 0) { fail("n_dims must be a positive multiple of n_dims_per_code"); return false; }
    if ((n_dims / dpc) * n_centroids * 4 > 160 * 1024) { fail("PQ table exceeds LDS"); return false; }
    return true;
}

}  // namespace

extern "C" {

mse_pq_trainer* mse_pq_trainer_new(size_t n_dims, size_t n_dims_per_code, size_t n_centroids) {
    if (!shape_ok(n_dims, n_dims_per_code, n_centroids)) return nullptr;
    if (n_dims > 32768) { fail("pq_trainer: n_dims is too large"); return nullptr; }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); fail("pq_trainer: no HIP device"); return nullptr; }
    mse_pq_trainer* tr = new (std::nothrow) mse_pq_trainer();
    if (!tr) { fail("out of host memory"); return nullptr; }
    tr->d = n_dims; tr->dpc = n_dims_per_code; tr->n_chunks = n_dims / n_dims_per_code; tr->n_cells = n_centroids; tr->device = device;
    const size_t pbytes = n_centroids * n_dims * 4;
    if (tr->m.ensure(pbytes) || tr->v.ensure(pbytes) || tr->grad.ensure(pbytes) || hipMemset(tr->m.p, 0, pbytes) != hipSuccess || hipMemset(tr->v.p, 0, pbytes) != hipSuccess) {
        delete tr;
        fail("pq_trainer: device allocation failed");
        return nullptr;
    }
    return tr;
}

void mse_pq_trainer_free(mse_pq_trainer* tr) { delete tr; }

static int sample_set(mse_pq_trainer* tr) {
    if (ensure_slots(tr)) return -1;
    return rerotate(tr);
}

int mse_pq_trainer_set_sample_f32(mse_pq_trainer* tr, const float* x, size_t n) {
    if (scope_check(tr, "pq_trainer_set_sample_f32")) return -1;
    if (!x) return fail("pq_trainer_set_sample_f32: null rows");
    if (n < tr->n_cells) return fail("pq_trainer_set_sample: fewer rows than centroids");
    if (n > 0xFFFFFFFEull) return fail("pq_trainer_set_sample: too many rows");
    if (tr->x32.ensure(n * tr->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->x32.p, x, n * tr->d * 4, hipMemcpyHostToDevice));
    tr->x16.release();
    tr->n = n; tr->from_base = false;
    return sample_set(tr);
}

int mse_pq_trainer_set_sample_base(mse_pq_trainer* tr, const mse_base* b, const uint32_t* ids, size_t n) {
    if (scope_check(tr, "pq_trainer_set_sample_base")) return -1;
    if (!b || !ids) return fail("pq_trainer_set_sample_base: null base or ids");
    if (b->d != tr->d) return fail("pq_trainer_set_sample_base: base width differs from the trainer's");
    if (b->device != tr->device) return fail("pq_trainer_set_sample_base: the base lives on another device");
    if (n < tr->n_cells) return fail("pq_trainer_set_sample: fewer rows than centroids");
    if (n > 0xFFFFFFFEull) return fail("pq_trainer_set_sample: too many rows");
    for (size_t i = 0; i < n; i++)
        if (ids[i] >= b->n) return fail("pq_trainer_set_sample_base: row id " + std::to_string(ids[i]) + " is not below " + std::to_string(b->n));
    if (tr->ids.ensure(n * 4) || tr->x16.ensure(n * tr->d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->ids.p, ids, n * 4, hipMemcpyHostToDevice));
    if (launch_gather_rows_f16(b->dev, tr->ids.as<uint32_t>(), n, (int)tr->d, tr->x16.as<uint16_t>(), nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    tr->x32.release();
    tr->n = n; tr->from_base = true;
    return sample_set(tr);
}

int mse_pq_trainer_set_transform(mse_pq_trainer* tr, const float* T) {
    if (scope_check(tr, "pq_trainer_set_transform")) return -1;
    if (!T) return fail("pq_trainer_set_transform: null matrix");
    if (tr->T.ensure(tr->d * tr->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->T.p, T, tr->d * tr->d * 4, hipMemcpyHostToDevice));
    tr->have_T = true;
    if (rerotate(tr)) return -1;
    return rotate_moment(tr);
}

int mse_pq_trainer_set_centroids(mse_pq_trainer* tr, const float* centroids) {
    if (scope_check(tr, "pq_trainer_set_centroids")) return -1;
    if (!centroids) return fail("pq_trainer_set_centroids: null array");
    if (tr->cent.ensure(tr->n_cells * tr->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->cent.p, centroids, tr->n_cells * tr->d * 4, hipMemcpyHostToDevice));
    tr->have_cent = true;
    return 0;
}

int mse_pq_trainer_set_query_moment(mse_pq_trainer* tr, const float* C0) {
    if (scope_check(tr, "pq_trainer_set_query_moment")) return -1;
    if (!C0) return fail("pq_trainer_set_query_moment: null matrix");
    if (tr->C0.ensure(tr->d * tr->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(tr->C0.p, C0, tr->d * tr->d * 4, hipMemcpyHostToDevice));
    tr->have_C0 = true;
    return rotate_moment(tr);
}

int mse_pq_trainer_kmeans(mse_pq_trainer* tr, size_t iters, uint64_t* empty_cells) {
    if (scope_check(tr, "pq_trainer_kmeans") || need_state(tr, "pq_trainer_kmeans", false)) return -1;
    const size_t per = tr->n_chunks * tr->n_cells * tr->dpc, n_counts = tr->n_chunks * tr->n_cells;
    if (ensure_slots(tr) || tr->sums.ensure(std::max(row_chunks(tr), (size_t)1) * per * 8) || tr->counts.ensure(n_counts * 8)) return -1;
    unsigned long long empty = 0;
    for (size_t it = 0; it < iters; it++) {
        if (assign(tr)) return -1;
        MSE_HIP_TRY(hipMemsetAsync(tr->sums.p, 0, per * 8, nullptr));
        MSE_HIP_TRY(hipMemsetAsync(tr->counts.p, 0, n_counts * 8, nullptr));
        MSE_HIP_TRY(hipMemsetAsync(slot_empty(tr), 0, 8, nullptr));
        AccumulateArgs a;
        a.v = tr->xr.as<float>(); a.n = tr->n; a.w = (int)tr->dpc; a.v_stride = tr->d; a.v_step = (int)tr->dpc;
        a.code = tr->codes.as<uint8_t>(); a.code_stride = tr->n_chunks; a.code_step = 1;
        a.n_cells = (int)tr->n_cells; a.n_slices = (int)tr->n_chunks; a.E = slot_E(tr, 0);
        a.sums = tr->sums.as<long long>(); a.sums_step = tr->n_cells * tr->dpc; a.counts = tr->counts.as<unsigned long long>();
        if (launch_accumulate_by_code(a, nullptr) ||
            launch_kmeans_update(tr->sums.as<long long>(), tr->counts.as<unsigned long long>(), slot_E(tr, 0), (int)tr->n_chunks, (int)tr->n_cells,
                                 (int)tr->dpc, (int)tr->d, tr->cent.as<float>(), slot_empty(tr), nullptr)) return -1;
    }
    MSE_HIP_TRY(hipMemcpy(&empty, slot_empty(tr), 8, hipMemcpyDeviceToHost));
    if (empty_cells) *empty_cells = iters ? (uint64_t)empty : 0;
    return 0;
}

int mse_pq_trainer_refine(mse_pq_trainer* tr, size_t steps, float lr, float beta1, float beta2, float eps, double* loss) {
    if (scope_check(tr, "pq_trainer_refine") || need_state(tr, "pq_trainer_refine", true)) return -1;
    if (steps == 0) return 0;
    if (!loss) return fail("pq_trainer_refine: null loss array");
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(lr >= 0.0f) || !(eps >= 0.0f)) return fail("pq_trainer_refine: invalid Adam parameters");
    if (tr->loss.ensure(steps * 8)) return -1;
    const size_t per = tr->n_chunks * tr->n_cells * tr->dpc;
    for (size_t s = 0; s < steps; s++) {
        const bool last = s + 1 == steps;
        StepEvents ev;
        if (forward(tr, true, tr->loss.as<double>() + s, last ? &ev : nullptr)) return -1;
        tr->t += 1;
        const double bc1 = 1.0 - std::pow((double)beta1, (double)tr->t), bc2 = 1.0 - std::pow((double)beta2, (double)tr->t);
        AdamArgs a;
        a.sums = tr->sums.as<long long>(); a.slot_stride = per; a.E = slot_E(tr, 2); a.n_slots = (int)row_chunks(tr); a.n = tr->n;
        a.n_chunks = (int)tr->n_chunks; a.n_cells = (int)tr->n_cells; a.dpc = (int)tr->dpc; a.d = (int)tr->d;
        a.centroids = tr->cent.as<float>(); a.m = tr->m.as<float>(); a.v = tr->v.as<float>(); a.grad = tr->grad.as<float>();
        a.beta1 = beta1; a.beta2 = beta2; a.step_size = (float)((double)lr / bc1); a.bc2_sqrt = (float)std::sqrt(bc2); a.eps = eps;
        hipEvent_t e0 = last ? ev.mark() : nullptr;
        if (launch_adam_step(a, nullptr)) return -1;
        tr->have_grad = true;
        hipEvent_t e1 = last ? ev.mark() : nullptr;
        if (last) {
            MSE_HIP_TRY(hipDeviceSynchronize());
            tr->ms[3] = span(e0, e1);
        }
    }
    MSE_HIP_TRY(hipMemcpy(loss, tr->loss.p, steps * 8, hipMemcpyDeviceToHost));
    return take_error(tr, "pq_trainer_refine");
}

int mse_pq_trainer_loss(mse_pq_trainer* tr, double* loss) {
    if (scope_check(tr, "pq_trainer_loss") || need_state(tr, "pq_trainer_loss", true)) return -1;
    if (!loss) return fail("pq_trainer_loss: null result");
    if (tr->loss.ensure(8)) return -1;
    if (forward(tr, false, tr->loss.as<double>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(loss, tr->loss.p, 8, hipMemcpyDeviceToHost));
    return take_error(tr, "pq_trainer_loss");
}

int mse_pq_trainer_cross(mse_pq_trainer* tr, double* M) {
    if (scope_check(tr, "pq_trainer_cross") || need_state(tr, "pq_trainer_cross", false)) return -1;
    if (!M) return fail("pq_trainer_cross: null result");
    const size_t d = tr->d, sig = tr->n_chunks * tr->n_cells * d;
    if (tr->sigma.ensure(sig * 8) || tr->M.ensure(d * d * 8)) return -1;
    if (assign(tr)) return -1;
    MSE_HIP_TRY(hipMemsetAsync(tr->sigma.p, 0, sig * 8, nullptr));
    AccumulateArgs a;
    a.v = tr->xr.as<float>(); a.n = tr->n; a.w = (int)d; a.v_stride = d; a.v_step = 0;
    a.code = tr->codes.as<uint8_t>(); a.code_stride = tr->n_chunks; a.code_step = 1;
    a.n_cells = (int)tr->n_cells; a.n_slices = (int)tr->n_chunks; a.E = slot_E(tr, 0);
    a.sums = tr->sigma.as<long long>(); a.sums_step = tr->n_cells * d;
    if (launch_accumulate_by_code(a, nullptr) ||
        launch_cross_matrix(tr->sigma.as<long long>(), slot_E(tr, 0), tr->cent.as<float>(), (int)tr->n_cells, (int)tr->dpc, (int)d, tr->M.as<double>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(M, tr->M.p, d * d * 8, hipMemcpyDeviceToHost));
    return 0;
}

int mse_pq_trainer_read(mse_pq_trainer* tr, float* centroids, float* transform) {
    if (scope_check(tr, "pq_trainer_read")) return -1;
    if (centroids) {
        if (!tr->have_cent) return fail("pq_trainer_read: no centroids set");
        MSE_HIP_TRY(hipMemcpy(centroids, tr->cent.p, tr->n_cells * tr->d * 4, hipMemcpyDeviceToHost));
    }
    if (transform) {
        if (!tr->have_T) return fail("pq_trainer_read: no transform set");
        MSE_HIP_TRY(hipMemcpy(transform, tr->T.p, tr->d * tr->d * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

int mse_pq_trainer_codes(mse_pq_trainer* tr, uint8_t* codes) {
    if (scope_check(tr, "pq_trainer_codes") || need_state(tr, "pq_trainer_codes", false)) return -1;
    if (!codes) return fail("pq_trainer_codes: null result");
    if (assign(tr)) return -1;
    MSE_HIP_TRY(hipMemcpy(codes, tr->codes.p, tr->n * tr->n_chunks, hipMemcpyDeviceToHost));
    return 0;
}

int mse_pq_trainer_rotated_rows(mse_pq_trainer* tr, const uint32_t* rows, size_t m, float* out) {
    if (scope_check(tr, "pq_trainer_rotated_rows")) return -1;
    if (!tr->n || !tr->have_T) return fail("pq_trainer_rotated_rows: sample and transform must be set");
    if ((!rows || !out) && m) return fail("pq_trainer_rotated_rows: null array");
    for (size_t i = 0; i < m; i++)
        if (rows[i] >= tr->n) return fail("pq_trainer_rotated_rows: row " + std::to_string(rows[i]) + " is not below " + std::to_string(tr->n));
    for (size_t i = 0; i < m; i++)
        MSE_HIP_TRY(hipMemcpy(out + i * tr->d, tr->xr.as<float>() + (size_t)rows[i] * tr->d, tr->d * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_pq_trainer_gradient(mse_pq_trainer* tr, float* grad) {
    if (scope_check(tr, "pq_trainer_gradient")) return -1;
    if (!grad) return fail("pq_trainer_gradient: null result");
    if (!tr->have_grad) return fail("pq_trainer_gradient: no refine step has run");
    MSE_HIP_TRY(hipMemcpy(grad, tr->grad.p, tr->n_cells * tr->d * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_pq_trainer_adam_state(mse_pq_trainer* tr, float* m, float* v, uint64_t* t) {
    if (scope_check(tr, "pq_trainer_adam_state")) return -1;
    const size_t bytes = tr->n_cells * tr->d * 4;
    if (m) MSE_HIP_TRY(hipMemcpy(m, tr->m.p, bytes, hipMemcpyDeviceToHost));
    if (v) MSE_HIP_TRY(hipMemcpy(v, tr->v.p, bytes, hipMemcpyDeviceToHost));
    if (t) *t = tr->t;
    return 0;
}

int mse_pq_trainer_set_adam_state(mse_pq_trainer* tr, const float* m, const float* v, uint64_t t) {
    if (scope_check(tr, "pq_trainer_set_adam_state")) return -1;
    if (!m || !v) return fail("pq_trainer_set_adam_state: null moments");
    const size_t bytes = tr->n_cells * tr->d * 4;
    MSE_HIP_TRY(hipMemcpy(tr->m.p, m, bytes, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(tr->v.p, v, bytes, hipMemcpyHostToDevice));
    tr->t = t;
    return 0;
}

mse_pq* mse_pq_trainer_finish(mse_pq_trainer* tr) {
    if (!tr) { fail("pq_trainer_finish: null trainer"); return nullptr; }
    if (!tr->have_cent || !tr->have_T) { fail("pq_trainer_finish: centroids and transform must be set"); return nullptr; }
    std::vector<float> c(tr->n_cells * tr->d), T(tr->d * tr->d);
    if (mse_pq_trainer_read(tr, c.data(), T.data())) return nullptr;
    return mse_pq_load(c.data(), tr->n_cells, T.data(), tr->d, tr->dpc);
}

int mse_pq_trainer_timing(mse_pq_trainer* tr, float* ms) {
    if (scope_check(tr, "pq_trainer_timing")) return -1;
    if (!ms) return fail("pq_trainer_timing: null result");
    for (int i = 0; i < 4; i++) ms[i] = tr->ms[i];
    return 0;
}

int mse_debug_pq_trainer_chunk_rows(mse_pq_trainer* tr, size_t rows) {
    if (scope_check(tr, "debug_pq_trainer_chunk_rows")) return -1;
    if (rows == 0 || rows > ((size_t)1 << 20)) return fail("debug_pq_trainer_chunk_rows: 1 .. 2^20 rows");
    tr->chunk_rows = rows;
    tr->slots.release();
    tr->n_slots = 0;
    if (ensure_slots(tr)) return -1;
    return rerotate(tr);   // slot 0 (the exponent of X') lives in the slots
}

int mse_debug_accumulate_by_code(const float* v, size_t n, size_t w, const uint8_t* code, size_t n_cells, int64_t* sums, int* E) {
    if (!v || !code || !sums || !E) return fail("debug_accumulate_by_code: null array");
    if (n == 0 || n > 0xFFFFFFFEull || w == 0 || w > 65536) return fail("debug_accumulate_by_code: n and w must be positive (w <= 65536)");
    if (n_cells == 0 || n_cells > 256) return fail("debug_accumulate_by_code: 1..256 cells");
    for (size_t i = 0; i < n; i++)
        if (code[i] >= n_cells) return fail("debug_accumulate_by_code: a code is not below n_cells");
    DevBuf dv, dc, ds, dm;
    if (dv.ensure(n * w * 4) || dc.ensure(n) || ds.ensure(n_cells * w * 8) || dm.ensure(16)) return -1;
    MSE_HIP_TRY(hipMemcpy(dv.p, v, n * w * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dc.p, code, n, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemset(ds.p, 0, n_cells * w * 8));
    MSE_HIP_TRY(hipMemset(dm.p, 0, 16));
    uint32_t* max_bits = dm.as<uint32_t>();
    int* Ed = dm.as<int>() + 1;
    uint32_t* err = dm.as<uint32_t>() + 2;
    AccumulateArgs a;
    a.v = dv.as<float>(); a.n = n; a.w = (int)w; a.v_stride = w; a.code = dc.as<uint8_t>(); a.code_stride = 1;
    a.n_cells = (int)n_cells; a.E = Ed; a.sums = ds.as<long long>();
    if (launch_abs_max(dv.as<float>(), n * w, max_bits, nullptr) || launch_fixed_exponent(max_bits, n, Ed, err, nullptr)) return -1;
    uint32_t host[3] = {0, 0, 0};
    MSE_HIP_TRY(hipMemcpy(host, dm.p, 12, hipMemcpyDeviceToHost));
    if (host[2]) return fail("debug_accumulate_by_code: non-finite input");
    if (launch_accumulate_by_code(a, nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(sums, ds.p, n_cells * w * 8, hipMemcpyDeviceToHost));
    *E = (int)host[1];
    return 0;
}

int mse_debug_residual_gemm(const float* xr, const uint8_t* codes, const float* centroids, const float* Cm, size_t n, size_t n_dims,
                            size_t n_dims_per_code, size_t n_centroids, float* G, float* lrow) {
    if (!xr || !codes || !centroids || !Cm || !G || !lrow) return fail("debug_residual_gemm: null array");
    if (!shape_ok(n_dims, n_dims_per_code, n_centroids)) return -1;
    if (n == 0 || n > ((size_t)1 << 20) || n_dims > 32768) return fail("debug_residual_gemm: 1 .. 2^20 rows");
    const size_t d = n_dims, nc = d / n_dims_per_code;
    for (size_t i = 0; i < n * nc; i++)
        if (codes[i] >= n_centroids) return fail("debug_residual_gemm: a code is not below n_centroids");
    const int parts = residual_gemm_parts((int)d);
    DevBuf dx, dc, dcent, dC, dG, dp, dl;
    if (dx.ensure(n * d * 4) || dc.ensure(n * nc) || dcent.ensure(n_centroids * d * 4) || dC.ensure(d * d * 4) || dG.ensure(n * d * 4) ||
        dp.ensure(n * parts * 4) || dl.ensure(n * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(dx.p, xr, n * d * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dc.p, codes, n * nc, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dcent.p, centroids, n_centroids * d * 4, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemcpy(dC.p, Cm, d * d * 4, hipMemcpyHostToDevice));
    if (launch_residual_gemm(dx.as<float>(), dc.as<uint8_t>(), dcent.as<float>(), dC.as<float>(), n, (int)d, (int)n_dims_per_code, dG.as<float>(),
                             dp.as<float>(), dl.as<float>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(G, dG.p, n * d * 4, hipMemcpyDeviceToHost));
    MSE_HIP_TRY(hipMemcpy(lrow, dl.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
