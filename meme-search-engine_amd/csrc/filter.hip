// Row filters of the filtered brute-force search (include/mse.h mse_filter): the device bitmap, its compacted id list, and the two
// small kernels the filtered passes add around the existing ones (api.hip exact_pass / mfma_pass).  The filtered graph search's LIST
// regime (beam_search.hip list_run) adds two more: the bitmap of the rows that are allowed AND carry a url, and the descriptor bias of
// a list pass.
//
// Bitmap: one bit per row, LSB first, one u32 word per 32-row group (the group of the MFMA scan's epilogue), padded with zero words
// to a whole number of 256-row scan tiles.  Id list: the allowed rows in ascending order, built once per filter -- the exact pass and
// the sparse path score it instead of all rows, and a position in it orders as its id does, so (score desc, position asc) selection
// is (score desc, id asc) selection.
#include "common.h"
#include "kernels.h"

namespace mse {
namespace {

constexpr int CB = 256;   // words per compaction block (8192 rows)

__global__ void or_ids_kernel(uint32_t* __restrict__ words, const uint32_t* __restrict__ ids, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t id = ids[i];
        atomicOr(&words[id >> 5], 1u << (id & 31));
    }
}

// inclusive scan of v over the CB threads of the block (Hillis-Steele in LDS); returns this thread's inclusive prefix
__device__ uint32_t block_scan(uint32_t v, uint32_t* tmp) {
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int off = 1; off < CB; off <<= 1) {
        const uint32_t add = t >= off ? tmp[t - off] : 0u;
        __syncthreads();
        tmp[t] += add;
        __syncthreads();
    }
    const uint32_t r = tmp[t];
    __syncthreads();
    return r;
}

// set bits per block of CB words
__global__ __launch_bounds__(CB) void count_blocks_kernel(const uint32_t* __restrict__ words, size_t n_words, uint32_t* __restrict__ counts) {
    __shared__ uint32_t tmp[CB];
    const size_t w = (size_t)blockIdx.x * CB + threadIdx.x;
    const uint32_t c = w < n_words ? (uint32_t)__popc(words[w]) : 0u;
    const uint32_t s = block_scan(c, tmp);
    if (threadIdx.x == CB - 1) counts[blockIdx.x] = s;
}

// exclusive prefix of the block counts (one workgroup; each thread walks a contiguous chunk) and the total
__global__ __launch_bounds__(CB) void scan_blocks_kernel(const uint32_t* __restrict__ counts, size_t n_blocks,
                                                        unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long part[CB];
    const size_t per = (n_blocks + CB - 1) / CB;
    const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < n_blocks ? lo + per : n_blocks;
    unsigned long long s = 0;
    for (size_t b = lo; b < hi; b++) s += counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < CB; t++) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (size_t b = lo; b < hi; b++) { offsets[b] = run; run += counts[b]; }
}

__global__ __launch_bounds__(CB) void compact_kernel(const uint32_t* __restrict__ words, size_t n_words,
                                                    const unsigned long long* __restrict__ offsets, uint32_t* __restrict__ ids) {
    __shared__ uint32_t tmp[CB];
    const size_t w = (size_t)blockIdx.x * CB + threadIdx.x;
    uint32_t bits = w < n_words ? words[w] : 0u;
    const uint32_t c = (uint32_t)__popc(bits);
    size_t at = offsets[blockIdx.x] + block_scan(c, tmp) - c;
    while (bits) {
        const int b = __ffs(bits) - 1;
        ids[at++] = (uint32_t)(w * 32 + b);
        bits &= bits - 1;
    }
}

__global__ void expand_groups_masked_kernel(const uint32_t* __restrict__ parents, size_t par_stride, size_t n_par, int group,
                                            size_t n_rows, const uint32_t* __restrict__ words, size_t n_words,
                                            uint32_t* __restrict__ ids, size_t ids_stride, int nq) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_q = n_par * (size_t)group;
    if (i >= per_q * (size_t)nq) return;
    const size_t q = i / per_q, r = i % per_q;
    const uint32_t p = parents[q * par_stride + r / group];
    uint32_t id = ID_NONE;
    if (p != ID_NONE) {
        const size_t row = (size_t)p * group + (r % group);
        if (row < n_rows && (row >> 5) < n_words && ((words[row >> 5] >> (row & 31)) & 1u)) id = (uint32_t)row;
    }
    ids[q * ids_stride + r] = id;
}

__global__ void map_positions_kernel(uint32_t* __restrict__ sel, size_t n, const uint32_t* __restrict__ list) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = sel[i];
    if (p != ID_NONE) sel[i] = list[p];
}

// out[w] = words[w] with the bits of rows whose byte in has_url is zero cleared (rows at or past n_rows: cleared).  One thread per word;
// its 32 flag bytes are two 16-byte loads (has_url comes from hipMalloc: 256-byte aligned, and 32 w is a multiple of 32).
__global__ void and_flags_kernel(const uint32_t* __restrict__ words, size_t n_words, const uint8_t* __restrict__ has_url, size_t n_rows,
                                 uint32_t* __restrict__ out) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t in = words[w];
    uint32_t keep = 0u;
    const size_t r0 = w * 32;
    if (in && r0 + 32 <= n_rows) {
        const uint4 lo = *reinterpret_cast<const uint4*>(has_url + r0), hi = *reinterpret_cast<const uint4*>(has_url + r0 + 16);
        const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int b = 0; b < 4; b++) keep |= ((v[i] >> (8 * b)) & 0xffu) ? 1u << (4 * i + b) : 0u;
    } else if (in) {
        for (int b = 0; b < 32 && r0 + b < n_rows; b++) keep |= has_url[r0 + b] ? 1u << b : 0u;
    }
    out[w] = in & keep;
}

// out[w] = NOT deleted[w] for the rows below n_rows (deleted == null: all ones), zero past them: the live rows of a graph as a filter's
// bitmap (mse_graph_live_filter).  deleted has ceil(n_rows / 32) words, out n_words >= that (the filter's tile padding).
__global__ void live_words_kernel(const uint32_t* __restrict__ deleted, size_t n_rows, size_t n_words, uint32_t* __restrict__ out) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const size_t r0 = w * 32;
    uint32_t v = 0u;
    if (r0 < n_rows) {
        v = deleted ? ~deleted[w] : 0xffffffffu;
        if (r0 + 32 > n_rows) v &= 0xffffffffu >> (32 - (n_rows - r0));
    }
    out[w] = v;
}

// scores[j][p] += descriptor_product(scales[j], row ids[p]) for the nq (<= 8) queries of a list pass: per term the f32 product is
// truncated to fixed point, the terms are summed as integers (the beam kernel's bias(pt); src/query_disk_index.rs:135-142).  A row's
// descriptor bytes are read once for all queries.  The sum wraps like the reference's release build (unsigned add: no overflow trap).
__global__ void list_bias_kernel(const uint32_t* __restrict__ ids, size_t n, const uint8_t* __restrict__ desc, int n_desc,
                                 const float* __restrict__ scales, int nq, int64_t* __restrict__ scores, size_t stride) {
    __shared__ float s_sc[8 * 8];
    if (threadIdx.x < 64) s_sc[threadIdx.x] = (int)threadIdx.x < nq * n_desc ? scales[threadIdx.x] : 0.0f;
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint8_t* dp = desc + (size_t)ids[p] * n_desc;
    float dv[8];
    for (int t = 0; t < n_desc; t++) dv[t] = (float)dp[t];
    for (int j = 0; j < nq; j++) {
        int64_t r = 0;
        for (int t = 0; t < n_desc; t++) r += scale_dot_result(s_sc[j * n_desc + t] * dv[t]);
        scores[(size_t)j * stride + p] = (int64_t)((uint64_t)scores[(size_t)j * stride + p] + (uint64_t)r);
    }
}

// ---- filters as values (mse_filter_combine / _not / _from_descriptors / _from_scores / _from_bits_dev) -------------------------------
// Every kernel below writes all n_words words of the new bitmap (the tile padding included, as zeros) and no bit at or past n_rows.

// the bits of word w that speak for rows below n_rows
__device__ __forceinline__ uint32_t row_mask(size_t w, size_t n_rows) {
    const size_t r0 = w * 32;
    if (r0 >= n_rows) return 0u;
    return r0 + 32 > n_rows ? 0xffffffffu >> (32 - (n_rows - r0)) : 0xffffffffu;
}

// out[w] = a[w] OP b[w] over the rows below n_rows; an operand reads as zero at and past its own words.  OP: MSE_FILTER_AND .. _ANDNOT,
// 4 = NOT a (b unused).  One thread per word.
template <int OP>
__global__ void combine_words_kernel(const uint32_t* __restrict__ a, size_t a_words, const uint32_t* __restrict__ b, size_t b_words,
                                     size_t n_rows, size_t n_words, uint32_t* __restrict__ out) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t x = w < a_words ? a[w] : 0u;
    const uint32_t y = OP != 4 && w < b_words ? b[w] : 0u;
    const uint32_t v = OP == 0 ? x & y : OP == 1 ? x | y : OP == 2 ? x ^ y : OP == 3 ? x & ~y : ~x;
    out[w] = v & row_mask(w, n_rows);
}

// the two words of this wave's 64 rows, from each lane's verdict on its row; lane 0 stores them (8-byte aligned: the pair index is even)
__device__ __forceinline__ void store_ballot(bool pass, size_t pair, uint32_t* __restrict__ out) {
    const unsigned long long m = __ballot(pass);
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<uint2*>(out + pair * 2) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
}

// bit r = lo[j] <= desc[r][j] <= hi[j] for every j < n_desc (bounds: byte j of lo / hi).  One wave per 64 rows, one lane per row, a block
// of four waves per 256-row tile of the bitmap (grid = n_words / 8).  WORD: n_desc == 4, the row's bytes are one aligned 4-byte load.
template <bool WORD>
__global__ __launch_bounds__(256) void desc_range_kernel(const uint8_t* __restrict__ desc, int n_desc, size_t n_rows, uint64_t lo, uint64_t hi,
                                                         uint32_t* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool pass = r < n_rows;
    if (pass) {
        if (WORD) {
            const uint32_t v = reinterpret_cast<const uint32_t*>(desc)[r];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t x = (v >> (8 * j)) & 0xffu;
                pass = pass && x >= (uint32_t)((lo >> (8 * j)) & 0xffu) && x <= (uint32_t)((hi >> (8 * j)) & 0xffu);
            }
        } else {
            const uint8_t* dp = desc + r * (size_t)n_desc;
            for (int j = 0; j < n_desc; j++) {
                const uint32_t x = dp[j];
                pass = pass && x >= (uint32_t)((lo >> (8 * j)) & 0xffu) && x <= (uint32_t)((hi >> (8 * j)) & 0xffu);
            }
        }
    }
    store_ballot(pass, r >> 6, out);
}

// bit r = scores[r] >= threshold, AND the bit of `within` (null: all rows; zero at and past its words).  Same shape as desc_range_kernel.
__global__ __launch_bounds__(256) void score_threshold_kernel(const int64_t* __restrict__ scores, size_t n_rows, int64_t threshold,
                                                              const uint32_t* __restrict__ within, size_t within_words,
                                                              uint32_t* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool pass = r < n_rows && scores[r] >= threshold;
    if (pass && within) pass = (r >> 5) < within_words && ((within[r >> 5] >> (r & 31)) & 1u);
    store_ballot(pass, r >> 6, out);
}

// clears the bits at and past n_rows in the word that holds row n_rows (n_rows % 32 != 0)
__global__ void mask_tail_kernel(uint32_t* __restrict__ words, size_t n_rows) {
    if (blockIdx.x == 0 && threadIdx.x == 0) words[n_rows >> 5] &= (1u << (n_rows & 31)) - 1u;
}

// ---- a global filter cut into per-shard ones and back (mse_filter_slice / mse_filter_concat) ---------------------------------------------

// out[w] = rows first_row + 32 w .. first_row + 32 w + 31 of `in`: the funnel of in[w0 + w] and in[w0 + w + 1] shifted right by
// first_row & 31, w0 = first_row >> 5 (a 64-bit shift: shift 0 is no special case).  `in` reads as zero at and past its in_words words and
// at and past its in_rows rows; the result is masked to n_rows, so the tile padding comes out as zero words.  One thread per output word.
__global__ void slice_words_kernel(const uint32_t* __restrict__ in, size_t in_words, size_t in_rows, uint64_t first_row, size_t n_rows,
                                   size_t n_words, uint32_t* __restrict__ out) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t keep = row_mask(w, n_rows);
    uint32_t v = 0u;
    if (keep) {
        const size_t s = (size_t)(first_row >> 5) + w;
        const uint32_t lo = s < in_words ? in[s] & row_mask(s, in_rows) : 0u;
        const uint32_t hi = s + 1 < in_words ? in[s + 1] & row_mask(s + 1, in_rows) : 0u;
        v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (first_row & 31)) & keep;
    }
    out[w] = v;
}

// The inverse: ORs `part` (part_rows rows), shifted left by first_row & 31, into out from word first_row >> 5 on.  Thread j owns the
// destination word (first_row >> 5) + j -- the funnel of part[j - 1] and part[j] -- so a launch needs no atomics, and the parts of one
// bitmap are placed by one launch each on ONE stream: two parts that share a boundary word meet in launch order.  out is n_rows rows of a
// zero-initialised bitmap; nothing is written at or past them.  part_words + 1 threads, part_words = ceil(part_rows / 32).
__global__ void place_words_kernel(const uint32_t* __restrict__ part, size_t part_rows, uint64_t first_row, size_t n_rows,
                                   uint32_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t part_words = (part_rows + 31) / 32;
    if (j > part_words) return;
    const size_t dst = (size_t)(first_row >> 5) + j;
    const uint32_t keep = row_mask(dst, n_rows);
    if (!keep) return;
    const uint32_t cur = j < part_words ? part[j] & row_mask(j, part_rows) : 0u;
    const uint32_t prev = j > 0 ? part[j - 1] & row_mask(j - 1, part_rows) : 0u;
    const uint32_t v = (uint32_t)((((uint64_t)cur << 32) | prev) >> (32 - (first_row & 31))) & keep;
    if (v) out[dst] |= v;
}

}  // namespace

int launch_filter_slice(const uint32_t* in, size_t in_words, size_t in_rows, uint64_t first_row, size_t n_rows, size_t n_words, uint32_t* out,
                        hipStream_t stream) {
    if (n_words == 0) return 0;
    hipLaunchKernelGGL(slice_words_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, in, in_words, in_rows, first_row,
                       n_rows, n_words, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_place(const uint32_t* part, size_t part_rows, uint64_t first_row, size_t n_rows, uint32_t* out, hipStream_t stream) {
    if (part_rows == 0) return 0;
    if (first_row > n_rows || part_rows > n_rows - first_row) return fail("filter concat: a part reaches past the result's rows");
    const size_t threads = (part_rows + 31) / 32 + 1;
    hipLaunchKernelGGL(place_words_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, part, part_rows, first_row, n_rows, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_combine(const uint32_t* a, size_t a_words, const uint32_t* b, size_t b_words, int op, size_t n_rows, size_t n_words,
                          uint32_t* out, hipStream_t stream) {
    if (n_words == 0) return 0;
    const dim3 grid((unsigned)((n_words + 255) / 256)), block(256);
    switch (op) {
#define MSE_COMBINE(OP) case OP: hipLaunchKernelGGL(combine_words_kernel<OP>, grid, block, 0, stream, a, a_words, b, b_words, n_rows, n_words, out); break;
        MSE_COMBINE(0) MSE_COMBINE(1) MSE_COMBINE(2) MSE_COMBINE(3) MSE_COMBINE(4)
#undef MSE_COMBINE
        default: return fail("filter combine: unknown op");
    }
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_desc_range(const uint8_t* desc, int n_desc, size_t n_rows, uint64_t lo, uint64_t hi, size_t n_words, uint32_t* out,
                             hipStream_t stream) {
    if (n_words == 0) return 0;
    if (n_desc < 1 || n_desc > 8) return fail("filter from descriptors: 1 to 8 descriptor bytes per row");
    if (n_words % 8 || n_words * 32 < n_rows) return fail("filter from descriptors: the bitmap is not whole tiles over the rows");
    const dim3 grid((unsigned)(n_words / 8)), block(256);
    if (n_desc == 4) hipLaunchKernelGGL(desc_range_kernel<true>, grid, block, 0, stream, desc, n_desc, n_rows, lo, hi, out);
    else hipLaunchKernelGGL(desc_range_kernel<false>, grid, block, 0, stream, desc, n_desc, n_rows, lo, hi, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_score_threshold(const int64_t* scores, size_t n_rows, int64_t threshold, const uint32_t* within, size_t within_words,
                                  size_t n_words, uint32_t* out, hipStream_t stream) {
    if (n_words == 0) return 0;
    if (n_words % 8 || n_words * 32 < n_rows) return fail("filter from scores: the bitmap is not whole tiles over the rows");
    hipLaunchKernelGGL(score_threshold_kernel, dim3((unsigned)(n_words / 8)), dim3(256), 0, stream, scores, n_rows, threshold, within,
                       within_words, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_mask_tail(uint32_t* words, size_t n_rows, hipStream_t stream) {
    if (n_rows % 32 == 0) return 0;
    hipLaunchKernelGGL(mask_tail_kernel, dim3(1), dim3(64), 0, stream, words, n_rows);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_count(const uint32_t* words, size_t n_words, unsigned long long* count_dev, void* scratch, hipStream_t stream) {
    const size_t nb = std::max<size_t>((n_words + CB - 1) / CB, 1);
    if (nb > 0x7fffffffull) return fail("filter: too many rows");
    unsigned long long* offsets = reinterpret_cast<unsigned long long*>(scratch);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + nb);
    hipLaunchKernelGGL(count_blocks_kernel, dim3((unsigned)nb), dim3(CB), 0, stream, words, n_words, counts);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(CB), 0, stream, counts, nb, offsets, count_dev);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_write_ids(const uint32_t* words, size_t n_words, const void* scratch, uint32_t* ids_out, hipStream_t stream) {
    const size_t nb = std::max<size_t>((n_words + CB - 1) / CB, 1);
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)nb), dim3(CB), 0, stream, words, n_words,
                       reinterpret_cast<const unsigned long long*>(scratch), ids_out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_and_flags(const uint32_t* words, size_t n_words, const uint8_t* has_url, size_t n_rows, uint32_t* out, hipStream_t stream) {
    if (n_words == 0) return 0;
    hipLaunchKernelGGL(and_flags_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, words, n_words, has_url, n_rows, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_live(const uint32_t* deleted, size_t n_rows, size_t n_words, uint32_t* out, hipStream_t stream) {
    if (n_words == 0) return 0;
    hipLaunchKernelGGL(live_words_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, deleted, n_rows, n_words, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_list_bias(const uint32_t* ids, size_t n, const uint8_t* desc, int n_desc, const float* scales, int nq, int64_t* scores, size_t stride,
                     hipStream_t stream) {
    if (n == 0 || nq == 0) return 0;
    if (nq > 8 || n_desc < 1 || n_desc > 8) return fail("list bias: at most 8 queries and 8 descriptors");
    hipLaunchKernelGGL(list_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ids, n, desc, n_desc, scales, nq, scores, stride);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_filter_or_ids(uint32_t* words, size_t n_words, const uint32_t* ids, size_t n, hipStream_t stream) {
    (void)n_words;   // the caller has checked every id against the filter's length
    if (n == 0) return 0;
    const size_t blocks = std::min<size_t>((n + 255) / 256, 65535);
    hipLaunchKernelGGL(or_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, words, ids, n);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

size_t filter_compact_scratch_bytes(size_t n_words) {
    const size_t nb = std::max<size_t>((n_words + CB - 1) / CB, 1);
    return nb * 4 + nb * 8 + 8 + 16;
}

int launch_filter_compact(const uint32_t* words, size_t n_words, uint32_t* ids_out, unsigned long long* count_dev, void* scratch,
                          hipStream_t stream) {
    const size_t nb = std::max<size_t>((n_words + CB - 1) / CB, 1);
    if (nb > 0x7fffffffull) return fail("filter: too many rows");
    unsigned long long* offsets = reinterpret_cast<unsigned long long*>(scratch);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + nb);
    hipLaunchKernelGGL(count_blocks_kernel, dim3((unsigned)nb), dim3(CB), 0, stream, words, n_words, counts);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(CB), 0, stream, counts, nb, offsets, count_dev);
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)nb), dim3(CB), 0, stream, words, n_words, offsets, ids_out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_expand_groups_masked(const uint32_t* parents, size_t par_stride, size_t n_par, int group, size_t n_rows, const uint32_t* words,
                                size_t n_words, uint32_t* ids, size_t ids_stride, int nq, hipStream_t stream) {
    const size_t total = n_par * (size_t)group * (size_t)nq;
    if (total == 0) return 0;
    hipLaunchKernelGGL(expand_groups_masked_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, parents, par_stride, n_par,
                       group, n_rows, words, n_words, ids, ids_stride, nq);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_map_positions(uint32_t* sel, size_t n, const uint32_t* list, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(map_positions_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sel, n, list);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mse
