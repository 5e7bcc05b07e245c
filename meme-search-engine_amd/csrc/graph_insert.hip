// Insert new rows into freed slots of a live graph index (include/mse.h "insert rows into freed slots"): the other direction of
// graph_delete.hip.  Four steps under the graph's exclusive lock:
//   validate  insert_check_kernel    every slot in range, marked in the graph's deleted map and named once (a scratch bitmap catches
//                                    the second naming); `start` live and not a slot.  One error word comes out; nothing has changed.
//   stage     insert_stage_kernel    one wave per new row: the row to base[slot] in 16-byte pieces; its three norm quantities, summed as
//                                    row_norm_max_kernel (gen.hip) sums them, folded into the base's cached bound by atomicMax on the
//                                    float bits (non-negative floats order as unsigned integers); its PQ code -- quantised over the
//                                    contiguous staging slab by the launches mse_codes_quantize_base uses -- and descriptor bytes to
//                                    codes[slot] / desc[slot]; has_url[slot]; the slot's bit cleared in the deleted map (atomicAnd:
//                                    several slots share a word).
//   link      build_graph_on_device  (graph_build.hip) the body of mse_build_graph over order = slots, unchanged kernels, scratch kept
//                                    on the searcher.
// The staging slab is at most STAGE_ROWS rows, so the scratch does not grow with the size of an insert.
#include "../../include/mse.h"
#include "runtime.h"
#include <algorithm>
#include <cstring>
#include <mutex>

using namespace mse;

namespace {

constexpr size_t STAGE_ROWS = 16384;   // rows widened, transformed and quantised at a time (11.5 KB of scratch per row at d = 1152)
// the error word of insert_check_kernel
constexpr uint32_t IE_RANGE = 1u, IE_LIVE = 2u, IE_TWICE = 4u, IE_START_SLOT = 8u, IE_START_DEAD = 16u;

__global__ void insert_check_kernel(const uint32_t* __restrict__ slots, size_t m, uint32_t n, const uint32_t* __restrict__ deleted,
                                    uint32_t* __restrict__ seen /* zeroed, one bit per node */, uint32_t start, uint32_t* err) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && ((deleted[start >> 5] >> (start & 31)) & 1u)) atomicOr(err, IE_START_DEAD);   // (start < n: checked on the host)
    if (i >= m) return;
    const uint32_t v = slots[i];
    if (v >= n) { atomicOr(err, IE_RANGE); return; }
    const uint32_t bit = 1u << (v & 31);
    uint32_t e = 0;
    if (!(deleted[v >> 5] & bit)) e |= IE_LIVE;
    if (atomicOr(&seen[v >> 5], bit) & bit) e |= IE_TWICE;
    if (v == start) e |= IE_START_SLOT;
    if (e) atomicOr(err, e);
}

struct StageArgs {
    const uint16_t* rows; uint16_t* base; int d;      // rows: [m][d] staged; base: the index's rows
    const uint32_t* slots; uint32_t m;
    uint32_t* norm_bits;                              // the base's cached bound [3], or null (never measured: it stays unmeasured)
    const uint8_t* codes_src; uint8_t* codes; int cs; // [m][cs] -> codes[slot], or null
    const uint8_t* desc_src; uint8_t* desc; int nd;   // [m][nd] -> desc[slot], or null
    const uint8_t* url_src; uint8_t* has_url;         // [m] or null (= 1)
    uint32_t* deleted;
};

__global__ __launch_bounds__(256) void insert_stage_kernel(StageArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);   // one wave per new row
    if (i >= a.m) return;
    const uint32_t slot = a.slots[i];
    const int d = a.d;
    const uint4* src = reinterpret_cast<const uint4*>(a.rows + (size_t)i * d);
    uint4* dst = reinterpret_cast<uint4*>(a.base + (size_t)slot * d);
    for (int e = lane; e < d / 8; e += 64) dst[e] = src[e];
    if (a.norm_bits && lane < 4) {
        // row_norm_max_kernel's sums for one row: lane `part` of a quad takes every fourth 16-byte piece, low half before high half, then
        // the two exchanges inside the quad
        const uint4* xp = src + lane;
        float s = 0.0f, sub = 0.0f, mabs = 0.0f;
        for (int t = 0; t < d / 32; t++) {
            const uint4 x = xp[t * 4];
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[k] & 0xffffu));
                const float hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[k] >> 16));
                s = fmaf(lo, lo, s);
                s = fmaf(hi, hi, s);
                const float alo = fabsf(lo), ahi = fabsf(hi);
                if (alo < 6.103515625e-5f) sub += alo;
                if (ahi < 6.103515625e-5f) sub += ahi;
                if (alo == alo) mabs = fmaxf(mabs, alo);
                if (ahi == ahi) mabs = fmaxf(mabs, ahi);
            }
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        sub += __shfl_xor(sub, 1);
        sub += __shfl_xor(sub, 2);
        mabs = fmaxf(mabs, __shfl_xor(mabs, 1));
        mabs = fmaxf(mabs, __shfl_xor(mabs, 2));
        if (!(s == s)) s = __builtin_inff();
        if (lane == 0) {
            atomicMax(a.norm_bits, __float_as_uint(sqrtf(fmaxf(0.0f, s)) * 1.0001f));
            atomicMax(a.norm_bits + 1, __float_as_uint(fmaxf(0.0f, sub) * 1.0001f));
            atomicMax(a.norm_bits + 2, __float_as_uint(mabs));
        }
    }
    if (a.codes) {
        const uint8_t* cs_src = a.codes_src + (size_t)i * a.cs;
        uint8_t* cs_dst = a.codes + (size_t)slot * a.cs;
        if ((a.cs & 15) == 0) {   // (both slabs are 16-byte aligned: hipMalloc, and rows of a multiple of 16 bytes)
            for (int e = lane; e < a.cs / 16; e += 64) reinterpret_cast<uint4*>(cs_dst)[e] = reinterpret_cast<const uint4*>(cs_src)[e];
        } else {
            for (int e = lane; e < a.cs; e += 64) cs_dst[e] = cs_src[e];
        }
    }
    if (a.desc)
        for (int e = lane; e < a.nd; e += 64) a.desc[(size_t)slot * a.nd + e] = a.desc_src[(size_t)i * a.nd + e];
    if (lane == 0) {
        a.has_url[slot] = a.url_src ? a.url_src[i] : (uint8_t)1;
        atomicAnd(&a.deleted[slot >> 5], ~(1u << (slot & 31)));
    }
}

int insert_rows(const char* who, bool rows_on_device, mse_searcher* s, mse_graph* g, mse_pq* pq, mse_codes* codes, const uint32_t* slots, size_t m,
                const uint16_t* rows, const uint8_t* desc, const uint8_t* has_url, uint32_t start, const mse_build_config* cfg, size_t batch,
                uint64_t stats[2]) {
    const std::string pre = std::string(who) + ": ";
    if (!s || !s->base || !g || !cfg || !stats || (m && (!slots || !rows))) return fail(pre + "null argument");
    if (check_build_config(s, g, cfg, who)) return -1;
    const mse_base* b = s->base;
    if (codes) {
        if (codes->n != g->n) return fail(pre + "the codes speak for " + std::to_string(codes->n) + " rows, the graph has " + std::to_string(g->n));
        if (!pq) return fail(pre + "codes without the quantiser that makes them");
        if (pq->d != b->d || pq->n_chunks != codes->code_size) return fail(pre + "the quantiser does not match the rows (d) or the codes (chunks)");
        if (codes->n_desc && !desc) return fail(pre + "the codes carry descriptors: the new rows need theirs");
        if (!codes->n_desc && desc) return fail(pre + "descriptors given, but the codes carry none");
    } else {
        if (pq) return fail(pre + "a quantiser without the codes to write to");
        if (desc) return fail(pre + "descriptors given, but no codes to hold them");
    }
    if (start >= g->n) return fail(pre + "start is outside the graph");
    if (m > g->n) return fail(pre + "more rows than the graph has slots (a slot is named twice)");
    stats[0] = stats[1] = 0;
    if (rows_on_device && m && ((uintptr_t)rows & 15)) return fail(pre + "device rows must be 16-byte aligned");
    // exclusive: waits for the request-path calls in flight on the graph (they hold the lock shared) and keeps new ones out
    std::lock_guard<SharedExclusive> ex(g->entry_lock);
    if (m == 0) return 0;
    if (!g->deleted || !g->has_url || g->n_deleted < m) return fail(pre + "the graph has fewer deleted rows than slots were named (a slot is not deleted)");
    MSE_HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = s->stream;
    const size_t n = g->n, n_words = (n + 31) / 32, d = b->d;
    const size_t cs = codes ? codes->code_size : 0, nd = codes ? codes->n_desc : 0;

    // ---- validate: nothing below this block has run when it fails ------------------------------------------------------------
    DevBuf &d_slots = s->ins_scratch[0], &seen = s->ins_scratch[1], &d_rows = s->ins_scratch[2], &f32a = s->ins_scratch[3], &f32b = s->ins_scratch[4],
           &d_codes = s->ins_scratch[5], &d_desc = s->ins_scratch[6], &d_url = s->ins_scratch[7];
    const size_t step = std::min(m, STAGE_ROWS);
    if (d_slots.ensure(m * 4) || seen.ensure(n_words * 4 + 16) || (!rows_on_device && d_rows.ensure(step * d * 2)) ||
        (codes && (f32a.ensure(step * d * 4) || f32b.ensure(step * d * 4) || d_codes.ensure(step * cs))) || (nd && d_desc.ensure(step * nd)) ||
        (has_url && d_url.ensure(m)))
        return -1;
    uint32_t* err = seen.as<uint32_t>() + n_words;
    MSE_HIP_TRY(hipMemsetAsync(seen.p, 0, n_words * 4 + 16, st));
    MSE_HIP_TRY(hipMemcpyAsync(d_slots.p, slots, m * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(insert_check_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_slots.as<uint32_t>(), m, (uint32_t)n, g->deleted,
                       seen.as<uint32_t>(), start, err);
    MSE_HIP_TRY(hipGetLastError());
    uint32_t e = 0;
    MSE_HIP_TRY(hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, st));
    MSE_HIP_TRY(hipStreamSynchronize(st));
    if (e & IE_RANGE) return fail(pre + "a slot is outside the graph");
    if (e & IE_LIVE) return fail(pre + "a slot is not deleted (free slots are rows removed by mse_graph_delete_rows)");
    if (e & IE_TWICE) return fail(pre + "a slot is named twice");
    if (e & IE_START_SLOT) return fail(pre + "start is one of the slots");
    if (e & IE_START_DEAD) return fail(pre + "start is a deleted row");

    // ---- stage + restore ------------------------------------------------------------------------------------------------------
    uint32_t* norm_bits = nullptr;
    {
        std::lock_guard<std::mutex> ng(b->norm_mu);
        if (b->norm_ready) norm_bits = b->norm_bits_dev;
    }
    if (has_url) MSE_HIP_TRY(hipMemcpyAsync(d_url.p, has_url, m, hipMemcpyHostToDevice, st));
    for (size_t r0 = 0; r0 < m; r0 += step) {
        const size_t nr = std::min(step, m - r0);
        const uint16_t* src = rows + r0 * d;
        if (!rows_on_device) {
            MSE_HIP_TRY(hipMemcpyAsync(d_rows.p, src, nr * d * 2, hipMemcpyHostToDevice, st));
            src = d_rows.as<uint16_t>();
        }
        if (codes) {   // the code of a row = mse_pq_quantize_batch of its f32 widening: the launches of mse_codes_quantize_base
            if (launch_f16_to_f32(src, nr * d, f32a.as<float>(), st) || launch_pq_transform(pq->transform, (int)d, f32a.as<float>(), nr, f32b.as<float>(), st) ||
                launch_pq_quantize(pq->centroids, (int)pq->n_centroids, (int)d, (int)pq->dpc, f32b.as<float>(), nr, d_codes.as<uint8_t>(), st))
                return -1;
            if (nd) MSE_HIP_TRY(hipMemcpyAsync(d_desc.p, desc + r0 * nd, nr * nd, hipMemcpyHostToDevice, st));
        }
        StageArgs a{};
        a.rows = src; a.base = const_cast<uint16_t*>(b->dev); a.d = (int)d;
        a.slots = d_slots.as<uint32_t>() + r0; a.m = (uint32_t)nr;
        a.norm_bits = norm_bits;
        if (codes) { a.codes_src = d_codes.as<uint8_t>(); a.codes = codes->codes; a.cs = (int)cs; }
        if (nd) { a.desc_src = d_desc.as<uint8_t>(); a.desc = codes->desc; a.nd = (int)nd; }
        a.url_src = has_url ? d_url.as<uint8_t>() + r0 : nullptr; a.has_url = g->has_url;
        a.deleted = g->deleted;
        hipLaunchKernelGGL(insert_stage_kernel, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, st, a);
        MSE_HIP_TRY(hipGetLastError());
        // (no wait: the next piece's copies and launches follow this launch on the stream)
    }
    MSE_HIP_TRY(hipStreamSynchronize(st));   // the caller's host arrays have been read
    g->n_deleted -= m;

    // ---- link: mse_build_graph(order = slots) -------------------------------------------------------------------------------------
    // No whole-graph edge check here (2.5 GB of reads at 1e7 x 64): a graph that has a deleted row has been through delete_mark_kernel, which
    // validates every edge, and every writer of lists since (delete, build, stitch, insert) writes ids below n only.  The search and the
    // back-edge kernels still refuse an edge outside the index.
    if (batch == 0) batch = 64;
    size_t n_batches = 0;
    if (build_graph_on_device(s, g, d_slots.as<uint32_t>(), m, batch, start, cfg, s->ins_build, who, &n_batches)) return -1;
    stats[0] = m; stats[1] = n_batches;
    return 0;
}

}  // namespace

extern "C" {

int mse_graph_insert_rows(mse_searcher* s, mse_graph* g, mse_pq* pq_or_null, mse_codes* codes_or_null, const uint32_t* slots, size_t n_rows,
                          const uint16_t* rows_f16, const uint8_t* descriptors_or_null, const uint8_t* has_url_or_null, uint32_t start,
                          const mse_build_config* cfg, size_t batch, uint64_t stats[2]) {
    return insert_rows("graph_insert_rows", false, s, g, pq_or_null, codes_or_null, slots, n_rows, rows_f16, descriptors_or_null, has_url_or_null, start, cfg,
                       batch, stats);
}

int mse_graph_insert_rows_dev(mse_searcher* s, mse_graph* g, mse_pq* pq_or_null, mse_codes* codes_or_null, const uint32_t* slots, size_t n_rows,
                              const void* rows_f16_dev, const uint8_t* descriptors_or_null, const uint8_t* has_url_or_null, uint32_t start,
                              const mse_build_config* cfg, size_t batch, uint64_t stats[2]) {
    return insert_rows("graph_insert_rows_dev", true, s, g, pq_or_null, codes_or_null, slots, n_rows, reinterpret_cast<const uint16_t*>(rows_f16_dev),
                       descriptors_or_null, has_url_or_null, start, cfg, batch, stats);
}

int mse_debug_base_norm_bits(const mse_base* b, uint32_t out[3]) {
    if (!b || !out) return fail("debug_base_norm_bits: null argument");
    MSE_HIP_TRY(hipSetDevice(b->device));
    if (ensure_base_norm(b, hipStreamPerThread)) return -1;
    MSE_HIP_TRY(hipMemcpy(out, b->norm_bits_dev, 12, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
