// C ABI (include/mse.h): row groupings as objects, and the test hooks of the collapse kernel and of the graph request path's group step.
// The kernels are in group.hip; the searches that take a grouping are in bruteforce.hip, api_pq.hip and beam_search.hip.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <new>

namespace mse {

int check_groups(const mse_base* b, const mse_groups* g) {
    if (!g) return fail("null grouping");
    if (g->n_rows > b->n) return fail("grouping is longer than the base (" + std::to_string(g->n_rows) + " > " + std::to_string(b->n) + " rows)");
    if (g->device != b->device) return fail("grouping was made on another device than the base's");   // no silent copy
    return 0;
}

// The dense path keeps, per query of a pass, one table entry per row of the grouping: at most 1 GiB of it per pass, so fewer than the
// exact pass's 8 queries once the grouping is long (12-byte entries: 8 queries up to 1.1e7 rows, one query from 9e7 rows on).
int dense_pass_queries(size_t g_len, size_t bytes) {
    const size_t fit = ((size_t)1 << 30) / (std::max<size_t>(g_len, 1) * bytes);
    return (int)std::min<size_t>(8, std::max<size_t>(fit, 1));
}

}  // namespace mse

using namespace mse;

// validation, count and adoption of a device copy of the array (freed on failure)
static mse_groups* groups_finish(uint32_t* dev, size_t n_rows, int device) {
    DevBuf scratch;
    unsigned long long stats[3] = {0, 0, 0};
    const size_t n_words = (n_rows + 31) / 32;
    bool ok = scratch.ensure(24 + std::max<size_t>(n_words, 1) * 4) == 0;
    if (ok && hipMemsetAsync(scratch.p, 0, 24 + n_words * 4, nullptr) != hipSuccess) { ok = false; fail("groups: clearing the scratch failed"); }
    unsigned long long* stats_dev = scratch.as<unsigned long long>();
    uint32_t* present = reinterpret_cast<uint32_t*>(scratch.as<char>() + 24);
    ok = ok && launch_groups_validate(dev, n_rows, present, stats_dev, nullptr) == 0 && launch_groups_popcount(present, n_words, stats_dev, nullptr) == 0;
    if (ok && hipMemcpy(stats, stats_dev, 24, hipMemcpyDeviceToHost) != hipSuccess) { ok = false; fail("groups: the validation pass failed"); }
    if (ok && stats[0] > n_rows) {
        ok = false;
        fail("groups: group id " + std::to_string(stats[0] - 1) + " is not below n_rows " + std::to_string(n_rows) + " (and is not the no-group id)");
    }
    mse_groups* g = ok ? new (std::nothrow) mse_groups() : nullptr;
    if (ok && !g) fail("out of host memory");
    if (!g) { (void)hipFree(dev); return nullptr; }
    g->device = device; g->n_rows = n_rows; g->group_of = dev;
    g->count = (size_t)(stats[1] + stats[2]);
    return g;
}

static uint32_t* groups_alloc(size_t n_rows, int* device) {
    if (n_rows > 0xFFFFFFFEull) { fail("row ids are u32: too many rows"); return nullptr; }
    if (hipGetDevice(device) != hipSuccess) { (void)hipGetLastError(); fail("groups: no HIP device"); return nullptr; }
    uint32_t* dev = nullptr;
    if (hipMalloc((void**)&dev, std::max<size_t>(n_rows, 1) * 4) != hipSuccess) { (void)hipGetLastError(); fail("hipMalloc failed for the grouping"); return nullptr; }
    return dev;
}

extern "C" {

mse_groups* mse_groups_from_host(const uint32_t* group_of, size_t n_rows) {
    if (!group_of && n_rows) { fail("groups: null array"); return nullptr; }
    int device = 0;
    uint32_t* dev = groups_alloc(n_rows, &device);
    if (!dev) return nullptr;
    if (n_rows && hipMemcpy(dev, group_of, n_rows * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev); fail("groups: the upload failed"); return nullptr;
    }
    return groups_finish(dev, n_rows, device);
}

mse_groups* mse_groups_from_dev(const void* group_of_dev, size_t n_rows) {
    if (!group_of_dev && n_rows) { fail("groups: null array"); return nullptr; }
    if (n_rows) {   // the grouping belongs to the device the array lives on
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, group_of_dev) != hipSuccess || at.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            fail("groups_from_dev: not device memory"); return nullptr;
        }
        if (hipSetDevice(at.device) != hipSuccess) { fail("groups_from_dev: hipSetDevice failed"); return nullptr; }
    }
    int device = 0;
    uint32_t* dev = groups_alloc(n_rows, &device);
    if (!dev) return nullptr;
    if (n_rows && hipMemcpy(dev, group_of_dev, n_rows * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
        (void)hipFree(dev); fail("groups: the device copy failed"); return nullptr;
    }
    return groups_finish(dev, n_rows, device);
}

void mse_groups_free(mse_groups* g) {
    if (!g) return;
    if (g->group_of) (void)hipFree(g->group_of);
    delete g;
}
size_t mse_groups_len(const mse_groups* g) { return g ? g->n_rows : 0; }
size_t mse_groups_count(const mse_groups* g) { return g ? g->count : 0; }

int mse_groups_read(const mse_groups* g, uint32_t* out) {
    if (!g) return fail("groups_read: null grouping");
    if (g->n_rows == 0) return 0;
    if (!out) return fail("groups_read: null buffer");
    if (hipMemcpy(out, g->group_of, g->n_rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("groups_read: the read-back failed");
    return 0;
}

// The partition src induces on rows [first_row, first_row + n_rows), over local ids and canonically labelled (group.hip
// launch_groups_slice); validated and counted like any other grouping.  The scratch table goes when the call returns: groups_finish blocks
mse_groups* mse_groups_slice(const mse_groups* src, uint64_t first_row, size_t n_rows, int device) {
    if (!src) { fail("groups_slice: null grouping"); return nullptr; }
    if (n_rows == 0) { fail("groups_slice: n_rows must be positive"); return nullptr; }
    if (first_row > 0xFFFFFFFEull) { fail("groups_slice: row ids are u32: first_row is too large"); return nullptr; }
    int dev = src->device;
    if (device >= 0) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) { fail("groups_slice: device ordinal out of range"); return nullptr; }
        dev = device;
    }
    DeviceScope scope(dev);
    if (!scope.ok) { fail("groups_slice: hipSetDevice failed"); return nullptr; }
    const size_t m = first_row < src->n_rows ? std::min<size_t>(n_rows, src->n_rows - (size_t)first_row) : 0;   // the part inside src
    int made_on = 0;
    uint32_t* out = groups_alloc(m, &made_on);
    if (!out) return nullptr;
    DevBuf range, table;
    if (m) {
        const uint32_t* labels = src->group_of + first_row;
        if (dev != src->device) {   // another device: the slice's labels come over by ONE peer copy and are relabelled here
            if (range.ensure(m * 4)) { (void)hipFree(out); return nullptr; }
            if (hipMemcpyPeer(range.p, dev, labels, src->device, m * 4) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(out); fail("groups_slice: the peer copy failed"); return nullptr;
            }
            labels = range.as<uint32_t>();
        }
        if (table.ensure(src->n_rows * 4) || launch_groups_slice(labels, m, table.as<uint32_t>(), out, nullptr)) { (void)hipFree(out); return nullptr; }
    }
    return groups_finish(out, m, dev);
}

int mse_searcher_grouped_stats(const mse_searcher* s, uint32_t out[3]) {
    if (!s || !out) return fail("null argument");
    for (int i = 0; i < 3; i++) out[i] = s->last_grouped[i];
    return 0;
}

int mse_searcher_grouped_timing(mse_searcher* s, int enable, double out[4]) {
    if (!s) return fail("null searcher");
    for (int i = 0; out && i < 4; i++) out[i] = s->grp_ms[i];
    for (int i = 0; enable && i < 4; i++)
        if (!s->grp_ev[i]) MSE_HIP_TRY(hipEventCreate(&s->grp_ev[i]));
    if (enable == 2)
        for (int i = 0; i < 4; i++) s->grp_ms[i] = 0.0;
    s->grp_timing = enable != 0;
    return 0;
}

// test hook: the collapse kernel alone over ranked id lists the caller supplies (tests/test_gpu_grouped.py)
int mse_debug_collapse_topk(mse_searcher* s, const mse_groups* g, const uint32_t* ids, size_t n_list, size_t nq, size_t k, uint32_t* kept_pos,
                            uint32_t* n_reps) {
    if (!s) return fail("null searcher");
    if (!g) return fail("null grouping");
    if (!ids || !kept_pos || !n_reps) return fail("collapse_topk: null array");
    if (n_list == 0 || n_list > 2048) return fail("collapse_topk: 1..2048 entries per list");
    if (k == 0 || k > 2048) return fail("collapse_topk: k must be 1..2048");
    if (nq == 0 || nq > 65536) return fail("collapse_topk: 1..65536 queries");
    if (s->grp_ids.ensure(nq * n_list * 4) || s->grp_pos.ensure(nq * k * 4) || s->grp_reps.ensure(nq * 4)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(s->grp_ids.p, ids, nq * n_list * 4, hipMemcpyHostToDevice, s->stream));
    if (launch_collapse(s->grp_ids.as<uint32_t>(), n_list, n_list, g->group_of, g->n_rows, (int)k, (int)nq, s->grp_pos.as<uint32_t>(),
                        s->grp_reps.as<uint32_t>(), s->stream)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(kept_pos, s->grp_pos.p, nq * k * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(n_reps, s->grp_reps.p, nq * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

// test hook: the group step of the graph request path alone (group.hip launch_visited_group) over caller-supplied visited lists, in the
// buffers the request path keeps them in; the table form -- LDS or global memory -- is chosen by cap exactly as read_back_fused chooses it
int mse_debug_visited_collapse(mse_searcher* s, const mse_groups* g, uint32_t* ids, int64_t* scores, size_t cap, const uint32_t* n_visited, size_t nq) {
    if (!s) return fail("null searcher");
    if (!g) return fail("null grouping");
    if (!ids || !scores || !n_visited) return fail("visited_collapse: null array");
    if (cap == 0 || cap > 65536) return fail("visited_collapse: 1..65536 records per list");
    if (nq == 0 || nq > 65536) return fail("visited_collapse: 1..65536 queries");
    DevBuf &vi = s->pool[8], &vs = s->pool[9], &cnt = s->pool[10], &gt = s->pool[15];
    const size_t table_bytes = visited_group_scratch_bytes(nq, cap);
    if (vi.ensure(nq * cap * 4) || vs.ensure(nq * cap * 8) || cnt.ensure(nq * 4) || (table_bytes && gt.ensure(table_bytes))) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(vi.p, ids, nq * cap * 4, hipMemcpyHostToDevice, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(vs.p, scores, nq * cap * 8, hipMemcpyHostToDevice, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(cnt.p, n_visited, nq * 4, hipMemcpyHostToDevice, s->stream));
    if (launch_visited_group(vi.as<uint32_t>(), vs.as<long long>(), cap, cnt.as<uint32_t>(), nq, g->group_of, g->n_rows, gt.p, s->stream)) return -1;
    MSE_HIP_TRY(hipMemcpyAsync(ids, vi.p, nq * cap * 4, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipMemcpyAsync(scores, vs.p, nq * cap * 8, hipMemcpyDeviceToHost, s->stream));
    MSE_HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
}

}  // extern "C"
