// C ABI (include/mse.h): the shard partition -- kmeans.py:73-127 and src/dump_processor.rs:438-461 on the device -- and the medioid over
// an id list.  The kernels are in partition.hip; DESIGN.md 3.21 has the definitions.  Nothing is allocated before the arguments are checked:
// a handle is made without touching a device.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace mse;

struct mse_partitioner {
    size_t S = 0, d = 0;
    mse_partition_config cfg{};
    int device = -1;               // bound on the first call that touches a device
    // the sample
    size_t n = 0;
    DevBuf x16, ids;
    // annealing
    DevBuf st, c0, c1, nrm, sizes, fin, fin16, trace_F, trace_code;
    size_t trace_cap = 0;
    uint64_t t_queued = 0;         // iterations enqueued so far, the initial evaluation included (an upper bound of the device's t)
    bool annealed = false;
    // assignment
    DevBuf acen, scores[2], counts, assignment, bits, tmp_rows, dbg;
    size_t n_assigned = 0;
    bool have_acen = false;
    size_t chunk_rows = 65536;     // rows per pass of the scores-out form
    hipStream_t walk_stream = nullptr;
    hipEvent_t scored[2] = {nullptr, nullptr}, walked[2] = {nullptr, nullptr};
    float ms[3] = {0.0f, 0.0f, 0.0f};
    ~mse_partitioner() {
        for (int i = 0; i < 2; i++) {
            if (scored[i]) (void)hipEventDestroy(scored[i]);
            if (walked[i]) (void)hipEventDestroy(walked[i]);
        }
        if (walk_stream) (void)hipStreamDestroy(walk_stream);
    }
};

namespace {

int bind_device(mse_partitioner* p, const char* who) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return fail(std::string(who) + ": no HIP device"); }
    if (p->device < 0) p->device = device;
    if (p->device != device) return fail(std::string(who) + ": the handle belongs to another device");
    return 0;
}

// grow a device buffer and keep its first `used` bytes
int grow_keep(DevBuf& b, size_t used, size_t want) {
    if (b.cap >= want) return 0;
    DevBuf bigger;
    if (bigger.ensure(std::max(want, b.cap * 2))) return -1;
    if (used) MSE_HIP_TRY(hipMemcpy(bigger.p, b.p, used, hipMemcpyDeviceToDevice));
    std::swap(b.p, bigger.p);
    std::swap(b.cap, bigger.cap);
    return 0;
}

PartitionAnnealArgs anneal_args(mse_partitioner* p) {
    PartitionAnnealArgs a{};
    a.st = p->st.as<PartitionDevState>();
    a.c[0] = p->c0.as<float>(); a.c[1] = p->c1.as<float>(); a.nrm = p->nrm.as<float>();
    a.sizes = p->sizes.as<unsigned long long>();
    a.trace_F = p->trace_F.as<unsigned long long>(); a.trace_code = p->trace_code.as<uint8_t>(); a.trace_cap = p->trace_cap;
    a.S = (int)p->S; a.d = (int)p->d; a.n = p->n;
    a.seed = p->cfg.seed; a.reroll_after = p->cfg.reroll_after;
    a.accept_decay = p->cfg.accept_decay; a.reject_decay = p->cfg.reject_decay; a.reroll_heat = p->cfg.reroll_heat; a.cap = p->cfg.temperature_cap;
    // the stop test in integers: F < n * stop_fraction with the fraction taken to six decimals
    a.stop_den = 1000000ull;
    a.stop_num = (unsigned long long)std::llround(p->cfg.stop_fraction * 1e6);
    return a;
}

// a fresh annealing state for the current sample: t = 0, nothing evaluated
int reset_anneal(mse_partitioner* p) {
    const size_t cb = p->S * p->d * 4;
    if (p->st.ensure(sizeof(PartitionDevState)) || p->c0.ensure(cb) || p->c1.ensure(cb) || p->nrm.ensure(cb) || p->sizes.ensure(2 * 64 * 8)) return -1;
    PartitionDevState st{};
    st.T = p->cfg.temperature0;
    MSE_HIP_TRY(hipMemcpy(p->st.p, &st, sizeof st, hipMemcpyHostToDevice));
    MSE_HIP_TRY(hipMemset(p->sizes.p, 0, 2 * 64 * 8));
    p->t_queued = 0;
    p->annealed = false;
    return 0;
}

int sample_checks(mse_partitioner* p, size_t n, const char* who) {
    if (n < p->S) return fail(std::string(who) + ": fewer rows than shards");
    if (n > 0xFFFFFFFEull) return fail(std::string(who) + ": too many rows");
    return 0;
}

PartitionScoreArgs sample_pass(mse_partitioner* p, const float* cen) {
    PartitionScoreArgs a;
    a.rows = p->x16.as<uint16_t>(); a.n = p->n; a.d = (int)p->d; a.S = (int)p->S; a.cen = cen;
    return a;
}

int upload_centroids(mse_partitioner* p, const float* centroids, const char* who) {
    if (!centroids) return fail(std::string(who) + ": null centroids");
    if (bind_device(p, who)) return -1;
    if (p->dbg.ensure(p->S * p->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(p->dbg.p, centroids, p->S * p->d * 4, hipMemcpyHostToDevice));
    return 0;
}

// the scores-out form over `rows` f16 rows in chunks, the walk of chunk c on its own stream while chunk c + 1 is scored
int assign_rows(mse_partitioner* p, const uint16_t* rows_dev, size_t rows, double fudge) {
    const size_t S = p->S;
    if (grow_keep(p->assignment, p->n_assigned * 2, (p->n_assigned + rows) * 2)) return -1;
    const size_t chunk = std::min(p->chunk_rows, rows);
    if (p->scores[0].ensure(chunk * S * 8) || p->scores[1].ensure(chunk * S * 8)) return -1;
    if (!p->walk_stream) {
        MSE_HIP_TRY(hipStreamCreateWithFlags(&p->walk_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            MSE_HIP_TRY(hipEventCreateWithFlags(&p->scored[i], hipEventDisableTiming));
            MSE_HIP_TRY(hipEventCreateWithFlags(&p->walked[i], hipEventDisableTiming));
        }
    }
    MSE_HIP_TRY(hipDeviceSynchronize());   // whatever wrote the rows and the centroids is done before the second stream reads them
    size_t c = 0;
    for (size_t r0 = 0; r0 < rows; r0 += chunk, c++) {
        const size_t m = std::min(chunk, rows - r0);
        const int buf = (int)(c & 1);
        if (c >= 2) MSE_HIP_TRY(hipStreamWaitEvent(nullptr, p->walked[buf], 0));   // the walk of chunk c - 2 has left this buffer
        PartitionScoreArgs a;
        a.rows = rows_dev + r0 * p->d; a.n = m; a.d = (int)p->d; a.S = (int)S; a.cen = p->acen.as<float>(); a.scores = p->scores[buf].as<double>();
        if (launch_partition_score(a, nullptr)) return -1;
        MSE_HIP_TRY(hipEventRecord(p->scored[buf], nullptr));
        MSE_HIP_TRY(hipStreamWaitEvent(p->walk_stream, p->scored[buf], 0));
        if (launch_partition_walk(p->scores[buf].as<double>(), m, (int)S, fudge, p->counts.as<unsigned long long>(), p->counts.as<unsigned long long>() + 64,
                                  p->assignment.as<uint8_t>() + (p->n_assigned + r0) * 2, p->walk_stream)) return -1;
        MSE_HIP_TRY(hipEventRecord(p->walked[buf], p->walk_stream));
    }
    MSE_HIP_TRY(hipStreamSynchronize(p->walk_stream));
    MSE_HIP_TRY(hipDeviceSynchronize());
    p->n_assigned += rows;
    return 0;
}

int assign_checks(mse_partitioner* p, size_t n, double fudge, const char* who) {
    if (!p->have_acen) return fail(std::string(who) + ": no centroids (mse_partition_anneal or mse_partition_set_centroids first)");
    if (!(fudge >= 0.0) || !(fudge <= 1e6)) return fail(std::string(who) + ": the balance fudge must be in [0, 1e6]");
    if (p->n_assigned + n > 0xFFFFFFFEull) return fail(std::string(who) + ": too many rows");
    return 0;
}

int ensure_counts(mse_partitioner* p) {
    if (p->counts.p) return 0;
    if (p->counts.ensure(65 * 8)) return -1;
    unsigned long long h[65] = {0};
    h[64] = 1;                                  // bal_count starts at 1 (dump_processor.rs:426)
    MSE_HIP_TRY(hipMemcpy(p->counts.p, h, sizeof h, hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

extern "C" {

void mse_partition_config_default(mse_partition_config* cfg) {
    if (!cfg) return;
    cfg->temperature0 = 1.0f; cfg->accept_decay = 0.999f; cfg->reject_decay = 0.9995f; cfg->reroll_heat = 1.1f; cfg->temperature_cap = 1.5f;
    cfg->reroll_after = 100; cfg->seed = 0; cfg->stop_fraction = 0.1;
}

mse_partitioner* mse_partition_new(size_t n_shards, size_t d, const mse_partition_config* cfg) {
    if (n_shards < 2 || n_shards > 64) { fail("partition: 2 .. 64 shards"); return nullptr; }
    if (d == 0 || d % 8 != 0 || d > (size_t)D_MAX) { fail("partition: the width must be a positive multiple of 8, at most " + std::to_string(D_MAX)); return nullptr; }
    mse_partition_config c;
    mse_partition_config_default(&c);
    if (cfg) c = *cfg;
    if (!(c.temperature0 > 0.0f) || !(c.accept_decay > 0.0f) || !(c.reject_decay > 0.0f) || !(c.reroll_heat > 0.0f) || !(c.temperature_cap > 0.0f) ||
        !(c.stop_fraction >= 0.0) || !(c.stop_fraction <= 64.0)) { fail("partition: invalid annealing parameters"); return nullptr; }
    mse_partitioner* p = new (std::nothrow) mse_partitioner();
    if (!p) { fail("out of host memory"); return nullptr; }
    p->S = n_shards; p->d = d; p->cfg = c;
    return p;
}

void mse_partition_free(mse_partitioner* p) { delete p; }

int mse_partition_set_sample_f16(mse_partitioner* p, const uint16_t* rows, size_t n) {
    if (!p) return fail("partition_set_sample_f16: null partitioner");
    if (!rows) return fail("partition_set_sample_f16: null rows");
    if (sample_checks(p, n, "partition_set_sample_f16") || bind_device(p, "partition_set_sample_f16")) return -1;
    if (p->x16.ensure(n * p->d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(p->x16.p, rows, n * p->d * 2, hipMemcpyHostToDevice));
    p->n = n;
    return reset_anneal(p);
}

int mse_partition_set_sample_base(mse_partitioner* p, const mse_base* b, const uint32_t* ids, size_t n) {
    if (!p) return fail("partition_set_sample_base: null partitioner");
    if (!b || !ids) return fail("partition_set_sample_base: null base or ids");
    if (b->d != p->d) return fail("partition_set_sample_base: base width differs from the partitioner's");
    if (sample_checks(p, n, "partition_set_sample_base")) return -1;
    for (size_t i = 0; i < n; i++)
        if (ids[i] >= b->n) return fail("partition_set_sample_base: row id " + std::to_string(ids[i]) + " is not below " + std::to_string(b->n));
    if (bind_device(p, "partition_set_sample_base")) return -1;
    if (b->device != p->device) return fail("partition_set_sample_base: the base lives on another device");
    if (p->ids.ensure(n * 4) || p->x16.ensure(n * p->d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(p->ids.p, ids, n * 4, hipMemcpyHostToDevice));
    if (launch_gather_rows_f16(b->dev, p->ids.as<uint32_t>(), n, (int)p->d, p->x16.as<uint16_t>(), nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    p->n = n;
    return reset_anneal(p);
}

int mse_partition_anneal(mse_partitioner* p, size_t iters) {
    if (!p) return fail("partition_anneal: null partitioner");
    if (!p->n) return fail("partition_anneal: no sample set");
    if (iters > ((size_t)1 << 32)) return fail("partition_anneal: too many iterations");
    if (bind_device(p, "partition_anneal")) return -1;
    const size_t have = p->t_queued ? p->t_queued - 1 : 0, want = have + iters;
    if (grow_keep(p->trace_F, have * 8, want * 8) || grow_keep(p->trace_code, have, want)) return -1;
    p->trace_cap = std::min(p->trace_F.cap / 8, p->trace_code.cap);
    const PartitionAnnealArgs a = anneal_args(p);
    PartitionScoreArgs pass = sample_pass(p, p->nrm.as<float>());
    pass.sizes = a.sizes;
    pass.stopped = &a.st->stopped;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t todo = iters + (p->t_queued == 0 ? 1 : 0);      // the first call evaluates the initial centroids before iteration 1
    for (size_t it = 0; it < todo; it++) {
        const bool timed = it + 1 == todo;
        if (timed) for (auto& e : ev) MSE_HIP_TRY(hipEventCreate(&e));
        if (timed) (void)hipEventRecord(ev[0], nullptr);
        if (launch_partition_candidate(a, nullptr)) return -1;
        if (timed) (void)hipEventRecord(ev[1], nullptr);
        if (launch_partition_score(pass, nullptr)) return -1;
        if (timed) (void)hipEventRecord(ev[2], nullptr);
        if (launch_partition_decide(a, nullptr)) return -1;
        if (timed) (void)hipEventRecord(ev[3], nullptr);
        p->t_queued += 1;
        if ((it & 255) == 255) {                           // the flag is polled; once it is set the launches are no-ops
            uint32_t stopped = 0;
            MSE_HIP_TRY(hipMemcpy(&stopped, &a.st->stopped, 4, hipMemcpyDeviceToHost));
            if (stopped) break;
        }
    }
    // the result: the current raw centroids normalised, their f16 rounding (centroids.bin) and its widening (the assignment's centroids)
    PartitionDevState st{};
    MSE_HIP_TRY(hipMemcpy(&st, p->st.p, sizeof st, hipMemcpyDeviceToHost));
    if (ev[3]) {
        for (int i = 0; i < 3; i++)
            if (hipEventElapsedTime(&p->ms[i], ev[i], ev[i + 1]) != hipSuccess) { (void)hipGetLastError(); p->ms[i] = 0.0f; }
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    const size_t cb = p->S * p->d;
    if (p->fin.ensure(cb * 4) || p->fin16.ensure(cb * 2) || p->acen.ensure(cb * 4)) return -1;
    if (launch_partition_normalise(a.c[st.cur & 1u], (int)p->S, (int)p->d, p->fin.as<float>(), p->fin16.as<uint16_t>(), p->acen.as<float>(), nullptr)) return -1;
    MSE_HIP_TRY(hipDeviceSynchronize());
    p->annealed = true;
    p->have_acen = true;
    return 0;
}

int mse_partition_state(mse_partitioner* p, mse_partition_status* out) {
    if (!p || !out) return fail("partition_state: null argument");
    if (!p->n) return fail("partition_state: no sample set");
    PartitionDevState st{};
    MSE_HIP_TRY(hipMemcpy(&st, p->st.p, sizeof st, hipMemcpyDeviceToHost));
    out->t = st.t ? st.t - 1 : 0; out->last_fitness = st.last; out->last_improvement = st.li; out->temperature = st.T; out->stopped = st.stopped;
    return 0;
}

int mse_partition_trace(mse_partitioner* p, size_t first, size_t n, uint64_t* F, uint8_t* code) {
    if (!p) return fail("partition_trace: null partitioner");
    mse_partition_status st;
    if (mse_partition_state(p, &st)) return -1;
    if (first > st.t || n > st.t - first) return fail("partition_trace: past the " + std::to_string(st.t) + " iterations run");
    if (n == 0) return 0;
    if (!F || !code) return fail("partition_trace: null result");
    MSE_HIP_TRY(hipMemcpy(F, p->trace_F.as<uint64_t>() + first, n * 8, hipMemcpyDeviceToHost));
    MSE_HIP_TRY(hipMemcpy(code, p->trace_code.as<uint8_t>() + first, n, hipMemcpyDeviceToHost));
    return 0;
}

int mse_partition_centroids(mse_partitioner* p, float* raw, float* normalised, uint16_t* f16) {
    if (!p) return fail("partition_centroids: null partitioner");
    if (!p->annealed) return fail("partition_centroids: mse_partition_anneal has not run on this sample");
    const size_t cb = p->S * p->d;
    if (raw) {
        PartitionDevState st{};
        MSE_HIP_TRY(hipMemcpy(&st, p->st.p, sizeof st, hipMemcpyDeviceToHost));
        MSE_HIP_TRY(hipMemcpy(raw, (st.cur & 1u) ? p->c1.p : p->c0.p, cb * 4, hipMemcpyDeviceToHost));
    }
    if (normalised) MSE_HIP_TRY(hipMemcpy(normalised, p->fin.p, cb * 4, hipMemcpyDeviceToHost));
    if (f16) MSE_HIP_TRY(hipMemcpy(f16, p->fin16.p, cb * 2, hipMemcpyDeviceToHost));
    return 0;
}

int mse_partition_set_centroids(mse_partitioner* p, const float* centroids) {
    if (!p) return fail("partition_set_centroids: null partitioner");
    if (!centroids) return fail("partition_set_centroids: null centroids");
    if (bind_device(p, "partition_set_centroids")) return -1;
    if (p->acen.ensure(p->S * p->d * 4)) return -1;
    MSE_HIP_TRY(hipMemcpy(p->acen.p, centroids, p->S * p->d * 4, hipMemcpyHostToDevice));
    p->have_acen = true;
    return 0;
}

int mse_partition_count(mse_partitioner* p, const float* centroids, uint64_t* sizes, uint8_t* top2) {
    if (!p) return fail("partition_count: null partitioner");
    if (!sizes) return fail("partition_count: null result");
    if (!p->n) return fail("partition_count: no sample set");
    if (upload_centroids(p, centroids, "partition_count")) return -1;
    DevBuf sz, t2;
    if (sz.ensure(2 * p->S * 8) || (top2 && t2.ensure(p->n * 2))) return -1;
    MSE_HIP_TRY(hipMemset(sz.p, 0, 2 * p->S * 8));
    PartitionScoreArgs a = sample_pass(p, p->dbg.as<float>());
    a.sizes = sz.as<unsigned long long>();
    a.top2 = top2 ? t2.as<uint8_t>() : nullptr;
    if (launch_partition_score(a, nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(sizes, sz.p, 2 * p->S * 8, hipMemcpyDeviceToHost));
    if (top2) MSE_HIP_TRY(hipMemcpy(top2, t2.p, p->n * 2, hipMemcpyDeviceToHost));
    return 0;
}

int mse_partition_scores(mse_partitioner* p, const float* centroids, double* scores) {
    if (!p) return fail("partition_scores: null partitioner");
    if (!scores) return fail("partition_scores: null result");
    if (!p->n) return fail("partition_scores: no sample set");
    if (upload_centroids(p, centroids, "partition_scores")) return -1;
    const size_t chunk = std::min(p->chunk_rows, p->n);
    if (p->scores[0].ensure(chunk * p->S * 8)) return -1;
    for (size_t r0 = 0; r0 < p->n; r0 += chunk) {
        const size_t m = std::min(chunk, p->n - r0);
        PartitionScoreArgs a = sample_pass(p, p->dbg.as<float>());
        a.rows += r0 * p->d; a.n = m; a.scores = p->scores[0].as<double>();
        if (launch_partition_score(a, nullptr)) return -1;
        MSE_HIP_TRY(hipMemcpy(scores + r0 * p->S, p->scores[0].p, m * p->S * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

int mse_partition_assign_f16(mse_partitioner* p, const uint16_t* rows, size_t n, double fudge) {
    if (!p) return fail("partition_assign_f16: null partitioner");
    if (!rows && n) return fail("partition_assign_f16: null rows");
    if (assign_checks(p, n, fudge, "partition_assign_f16")) return -1;
    if (n == 0) return 0;
    if (bind_device(p, "partition_assign_f16") || ensure_counts(p)) return -1;
    // host rows go up a slab at a time: the slab is the unit of the upload only, the walk carries on across slabs
    const size_t slab = std::min(n, (size_t)1 << 18);
    if (p->tmp_rows.ensure(slab * p->d * 2)) return -1;
    for (size_t r0 = 0; r0 < n; r0 += slab) {
        const size_t m = std::min(slab, n - r0);
        MSE_HIP_TRY(hipMemcpy(p->tmp_rows.p, rows + r0 * p->d, m * p->d * 2, hipMemcpyHostToDevice));
        if (assign_rows(p, p->tmp_rows.as<uint16_t>(), m, fudge)) return -1;
    }
    return 0;
}

int mse_partition_assign_base(mse_partitioner* p, const mse_base* b, size_t first, size_t n, double fudge) {
    if (!p) return fail("partition_assign_base: null partitioner");
    if (!b) return fail("partition_assign_base: null base");
    if (b->d != p->d) return fail("partition_assign_base: base width differs from the partitioner's");
    if (first > b->n || n > b->n - first) return fail("partition_assign_base: rows past the end of the base");
    if (assign_checks(p, n, fudge, "partition_assign_base")) return -1;
    if (n == 0) return 0;
    if (bind_device(p, "partition_assign_base") || ensure_counts(p)) return -1;
    if (b->device != p->device) return fail("partition_assign_base: the base lives on another device");
    return assign_rows(p, b->dev + first * p->d, n, fudge);
}

int mse_partition_assign_reset(mse_partitioner* p) {
    if (!p) return fail("partition_assign_reset: null partitioner");
    p->n_assigned = 0;
    p->counts.release();
    return 0;
}

int mse_partition_assignment(mse_partitioner* p, size_t first, size_t n, uint8_t* out) {
    if (!p) return fail("partition_assignment: null partitioner");
    if (first > p->n_assigned || n > p->n_assigned - first) return fail("partition_assignment: past the " + std::to_string(p->n_assigned) + " rows assigned");
    if (n == 0) return 0;
    if (!out) return fail("partition_assignment: null result");
    MSE_HIP_TRY(hipMemcpy(out, p->assignment.as<uint8_t>() + first * 2, n * 2, hipMemcpyDeviceToHost));
    return 0;
}

int mse_partition_counts(mse_partitioner* p, uint64_t* counts, uint64_t* n_assigned) {
    if (!p) return fail("partition_counts: null partitioner");
    if (n_assigned) *n_assigned = p->n_assigned;
    if (counts) {
        if (!p->counts.p) { for (size_t s = 0; s < p->S; s++) counts[s] = 0; return 0; }
        MSE_HIP_TRY(hipMemcpy(counts, p->counts.p, p->S * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

mse_filter* mse_partition_shard_filter(mse_partitioner* p, size_t s) {
    if (!p) { fail("partition_shard_filter: null partitioner"); return nullptr; }
    if (s >= p->S) { fail("partition_shard_filter: shard " + std::to_string(s) + " is not below " + std::to_string(p->S)); return nullptr; }
    if (!p->n_assigned) { fail("partition_shard_filter: no rows assigned"); return nullptr; }
    if (p->bits.ensure((p->n_assigned + 63) / 64 * 8)) return nullptr;
    if (launch_partition_shard_bits(p->assignment.as<uint8_t>(), p->n_assigned, (int)s, p->bits.as<uint32_t>(), nullptr)) return nullptr;
    return mse_filter_from_bits_dev(p->bits.p, p->n_assigned);   // (null stream, as the copy in there: ordered after the kernel)
}

int mse_partition_timing(mse_partitioner* p, float* ms) {
    if (!p || !ms) return fail("partition_timing: null argument");
    for (int i = 0; i < 3; i++) ms[i] = p->ms[i];
    return 0;
}

int mse_medioid_ids(const mse_base* b, const uint32_t* ids, size_t n_ids, uint32_t* id_out) {
    if (!b || !ids || !id_out) return fail("medioid_ids: null argument");
    if (n_ids == 0) return fail("medioid_ids: empty id list");
    if (n_ids > 0xFFFFFFFEull) return fail("medioid_ids: too many ids");
    if (b->d % 8) return fail("medioid_ids: d must be a multiple of 8");
    for (size_t i = 0; i < n_ids; i++)
        if (ids[i] >= b->n) return fail("medioid_ids: row id " + std::to_string(ids[i]) + " is not below " + std::to_string(b->n));
    // rows[ids] in list order as a vector list of their own, through mse_medioid's kernels: the same arithmetic in the same order
    DevBuf idb, rows;
    if (idb.ensure(n_ids * 4) || rows.ensure(n_ids * b->d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(idb.p, ids, n_ids * 4, hipMemcpyHostToDevice));
    if (launch_gather_rows_f16(b->dev, idb.as<uint32_t>(), n_ids, (int)b->d, rows.as<uint16_t>(), nullptr)) return -1;
    mse_base listed;
    listed.dev = rows.as<uint16_t>(); listed.n = n_ids; listed.d = b->d; listed.device = b->device;
    return mse_medioid(&listed, id_out);
}

int mse_debug_partition_noise(uint32_t seed, uint64_t key, size_t d, float* out) {
    if (!out) return fail("debug_partition_noise: null result");
    if (d == 0 || d % 8 != 0 || d > (size_t)D_MAX) return fail("debug_partition_noise: the width must be a positive multiple of 8");
    DevBuf o;
    if (o.ensure(d * 4)) return -1;
    if (launch_partition_noise(seed, key, (int)d, o.as<float>(), nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, o.p, d * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mse_debug_partition_normalise(const float* c, size_t n_rows, size_t d, float* out, uint16_t* f16_out) {
    if (!c || !out) return fail("debug_partition_normalise: null argument");
    if (n_rows == 0 || n_rows > 65535 || d == 0 || d > (size_t)D_MAX) return fail("debug_partition_normalise: 1 .. 65535 rows of 1 .. " + std::to_string(D_MAX) + " floats");
    DevBuf in, o, h;
    if (in.ensure(n_rows * d * 4) || o.ensure(n_rows * d * 4) || h.ensure(n_rows * d * 2)) return -1;
    MSE_HIP_TRY(hipMemcpy(in.p, c, n_rows * d * 4, hipMemcpyHostToDevice));
    if (launch_partition_normalise(in.as<float>(), (int)n_rows, (int)d, o.as<float>(), h.as<uint16_t>(), nullptr, nullptr)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, o.p, n_rows * d * 4, hipMemcpyDeviceToHost));
    if (f16_out) MSE_HIP_TRY(hipMemcpy(f16_out, h.p, n_rows * d * 2, hipMemcpyDeviceToHost));
    return 0;
}

int mse_debug_partition_chunk_rows(mse_partitioner* p, size_t rows) {
    if (!p) return fail("debug_partition_chunk_rows: null partitioner");
    if (rows == 0 || rows > ((size_t)1 << 20)) return fail("debug_partition_chunk_rows: 1 .. 2^20 rows");
    p->chunk_rows = rows;
    return 0;
}

}  // extern "C"
