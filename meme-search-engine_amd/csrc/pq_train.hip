// Codec training kernels: the device side of diskann/aopq_train.py:33-85 as bench_ann.train_codec_aopq reads it.
// The rotation and the assignment are pq.hip's launch_pq_transform / launch_pq_quantize; this file adds the order-free sum by code
// (k-means sums, gradient sums, the cross matrix, the loss), the residual GEMM G = R C on the f32-input matrix cores, the Adam step
// and the small kernels between them.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace mse {
namespace {

// ---- order-free sum -----------------------------------------------------------------------------------------------------------
// max |v| as float bits: non-negative floats order like their bit patterns, so an integer atomicMax is an exact, order-free maximum.
// The patterns of inf and NaN are at or above 0x7f800000 and win it: the exponent kernel below refuses them.
__global__ __launch_bounds__(256) void abs_max_kernel(const float* __restrict__ v, size_t count, uint32_t* __restrict__ out_bits) {
    uint32_t m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const uint32_t b = __float_as_uint(v[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    for (int o = 32; o; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out_bits, m);
}

// E = 61 - ceil(log2 n) - ex with vmax = f 2^ex, f in [0.5, 1) (ex = 0 for vmax = 0): every term |v 2^E| < 2^(61 - ceil(log2 n)), so n
// of them stay below 2^61 in int64.  Integer arithmetic on the bit pattern, subnormals included.
__global__ void fixed_exponent_kernel(const uint32_t* __restrict__ max_bits, unsigned long long n, int* __restrict__ E, uint32_t* __restrict__ err) {
    const uint32_t b = *max_bits;
    if (b >= 0x7f800000u) { atomicOr(err, 1u); *E = 0; return; }
    int ex = 0;
    if (b >> 23) ex = (int)(b >> 23) - 126;
    else if (b) ex = (31 - __clz((int)b)) - 148;
    int lg = 0;
    while (lg < 63 && (1ull << lg) < n) lg++;
    *E = 61 - lg - ex;
}

struct AccLaunch {
    const float* v; size_t n; int w; size_t v_stride; int v_step;      // slice z reads columns z * v_step .. + w of rows of v_stride floats
    const uint8_t* code; size_t code_stride; int code_step;           // ... with the code at code[row * code_stride + z * code_step]
    int n_cells; const int* E;
    unsigned long long* sums; size_t sums_step;                       // slice z adds into sums + z * sums_step, [n_cells][w]
    unsigned long long* counts;                                       // optional: members per cell, [z][n_cells]
    int cw; unsigned rows_per_block;
};

// One workgroup: rows_per_block rows x cw columns of one slice, summed per cell in LDS (one cell may hold every row: no global atomic
// per term), then one 64-bit integer atomic per touched (cell, column).  Integer adds commute: the result does not depend on the
// geometry or on the order the hardware picks.
__global__ __launch_bounds__(256) void accumulate_by_code_kernel(AccLaunch a) {
    extern __shared__ __attribute__((aligned(8))) unsigned long long acc_lds[];   // [n_cells][cw] sums | [n_cells] u32 counts
    uint32_t* cnt = reinterpret_cast<uint32_t*>(acc_lds + (size_t)a.n_cells * a.cw);
    const int z = blockIdx.z, c0 = blockIdx.y * a.cw;
    const int ncol = a.w - c0 < a.cw ? a.w - c0 : a.cw;
    const size_t r0 = (size_t)blockIdx.x * a.rows_per_block;
    const size_t r1 = r0 + a.rows_per_block < a.n ? r0 + a.rows_per_block : a.n;
    const bool counting = a.counts != nullptr && blockIdx.y == 0;
    for (int e = threadIdx.x; e < a.n_cells * a.cw; e += 256) acc_lds[e] = 0ull;
    for (int e = threadIdx.x; e < a.n_cells; e += 256) cnt[e] = 0u;
    __syncthreads();
    const double scale = __builtin_ldexp(1.0, *a.E);
    const unsigned total = (unsigned)(r1 - r0) * (unsigned)ncol;
    for (unsigned e = threadIdx.x; e < total; e += 256) {
        const unsigned rr = e / (unsigned)ncol, col = e % (unsigned)ncol;
        const size_t row = r0 + rr;
        const int cell = a.code[row * a.code_stride + (size_t)z * a.code_step];
        if (cell >= a.n_cells) continue;
        const float val = a.v[row * a.v_stride + (size_t)z * a.v_step + c0 + col];
        const long long q = __double2ll_rn((double)val * scale);    // exact scaling, then round-half-even
        if (q) atomicAdd(&acc_lds[cell * a.cw + col], (unsigned long long)q);
        if (counting && col == 0) atomicAdd(&cnt[cell], 1u);
    }
    __syncthreads();
    unsigned long long* out = a.sums + (size_t)z * a.sums_step;
    for (int e = threadIdx.x; e < a.n_cells * ncol; e += 256) {
        const int cell = e / ncol, col = e % ncol;
        const unsigned long long s = acc_lds[cell * a.cw + col];
        if (s) atomicAdd(&out[(size_t)cell * a.w + c0 + col], s);
    }
    if (counting)
        for (int e = threadIdx.x; e < a.n_cells; e += 256)
            if (cnt[e]) atomicAdd(&a.counts[(size_t)z * a.n_cells + e], (unsigned long long)cnt[e]);
}

// ---- k-means ------------------------------------------------------------------------------------------------------------------
// c[s][k] = (float)(((double)S / (double)count) 2^-E); a cell without members keeps its centroid and is counted
__global__ void kmeans_update_kernel(const long long* __restrict__ sums, const unsigned long long* __restrict__ counts, const int* __restrict__ E,
                                     int n_chunks, int n_cells, int dpc, int d, float* __restrict__ cent, unsigned long long* __restrict__ empty) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_chunks * n_cells * dpc) return;
    const int u = idx % dpc, k = (idx / dpc) % n_cells, s = idx / (dpc * n_cells);
    const unsigned long long c = counts[s * n_cells + k];
    if (c == 0) {
        if (u == 0) atomicAdd(empty, 1ull);
        return;
    }
    const double mean = ((double)sums[idx] / (double)c) * __builtin_ldexp(1.0, -*E);
    cent[(size_t)k * d + s * dpc + u] = (float)mean;
}

// ---- residual GEMM --------------------------------------------------------------------------------------------------------------
// G = R C with R = X' - Y formed while the A operand is loaded: 128 x 128 outputs per workgroup, k in steps of 32 through LDS, four
// waves of 2 x 2 tiles of v_mfma_f32_32x32x2_f32.  One wave owns an output from k = 0 to d - 1 and feeds the k pairs in ascending
// order, so every G[i][j] is the chain fma(r_k, C_kj, .) over k ascending -- the same bits run to run.  The next k step's operands are
// fetched into registers while the matrix cores work on this one.
using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int GM = 128, GN = 128, GK = 32;
constexpr int G_AS = GK + 1;      // A tile [row][k], odd stride: the 32 rows of a half-wave land in 32 banks
constexpr int G_BS = GN + 32;     // B tile [k][column]: the two k of a step are 32 banks apart

__device__ __forceinline__ float residual_at(const float* __restrict__ xr, const uint8_t* __restrict__ codes, const float* __restrict__ cent,
                                             size_t row, int k, int d, int dpc, int n_chunks) {
    const int c = codes[row * n_chunks + k / dpc];
    return __fsub_rn(xr[row * d + k], cent[(size_t)c * d + k]);
}

__global__ __launch_bounds__(256, 2) void residual_gemm_kernel(const float* __restrict__ xr, const uint8_t* __restrict__ codes,
                                                            const float* __restrict__ cent, const float* __restrict__ Cm, size_t n, int d, int dpc,
                                                            float* __restrict__ G, float* __restrict__ lpart, int n_part) {
    __shared__ float As[GM * G_AS];
    __shared__ float Bs[GK * G_BS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int j0 = blockIdx.x * GN;
    const size_t i0 = (size_t)blockIdx.y * GM;
    const int n_chunks = d / dpc;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
    float ra[16], rb[16];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int e = tid + 256 * r;
            const int kk = e & 31, row = e >> 5;
            const size_t gi = i0 + row;
            ra[r] = (gi < n && k0 + kk < d) ? residual_at(xr, codes, cent, gi, k0 + kk, d, dpc, n_chunks) : 0.0f;
            const int j = e & 127, kb = e >> 7;
            rb[r] = (k0 + kb < d && j0 + j < d) ? Cm[(size_t)(k0 + kb) * d + j0 + j] : 0.0f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += GK) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int e = tid + 256 * r;
            As[(e >> 5) * G_AS + (e & 31)] = ra[r];
            Bs[(e >> 7) * G_BS + (e & 127)] = rb[r];
        }
        __syncthreads();
        if (k0 + GK < d) fetch(k0 + GK);
#pragma unroll
        for (int t = 0; t < GK / 2; t++) {
            const float a0 = As[(wm * 64 + l31) * G_AS + 2 * t + lh];
            const float a1 = As[(wm * 64 + 32 + l31) * G_AS + 2 * t + lh];
            const float b0 = Bs[(2 * t + lh) * G_BS + wn * 64 + l31];
            const float b1 = Bs[(2 * t + lh) * G_BS + wn * 64 + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: G, and the wave's share of l_row = r . G_row -- per lane fma over its two columns (left tile first), then a fixed butterfly
    // over the 32 lanes that hold the row: partial (row, 64-column group), summed in ascending group order by lrow_kernel
#pragma unroll
    for (int mt = 0; mt < 2; mt++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const size_t row = i0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float p = 0.0f;
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
                const int col = j0 + wn * 64 + nt * 32 + l31;
                if (row < n && col < d) {
                    const float g = acc[mt][nt][r];
                    if (G) G[row * d + col] = g;
                    p = fmaf(residual_at(xr, codes, cent, row, col, d, dpc, n_chunks), g, p);
                }
            }
#pragma unroll
            for (int o = 16; o; o >>= 1) p = __fadd_rn(p, __shfl_xor(p, o));
            if (l31 == 0 && row < n) lpart[row * n_part + blockIdx.x * 2 + wn] = p;
        }
    }
}

__global__ void lrow_kernel(const float* __restrict__ lpart, int n_part, size_t n, float* __restrict__ lrow) {
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    float s = 0.0f;
    for (int c = 0; c < n_part; c++) s = __fadd_rn(s, lpart[row * n_part + c]);
    lrow[row] = s;
}

// L = ((double)S 2^-E) / n
__global__ void loss_finish_kernel(const long long* __restrict__ S, const int* __restrict__ E, double n, double* __restrict__ out) {
    *out = ((double)*S * __builtin_ldexp(1.0, -*E)) / n;
}

// ---- gradient and Adam ----------------------------------------------------------------------------------------------------------
// grad = (float)(sum over the row chunks, ascending, of (double)S_c 2^-E_c, times -2 / n) -- one chunk: (double)S 2^-E (-2 / n) -- then
// torch.optim.Adam's update, elementwise in f32 (step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the host)
struct AdamLaunch {
    const long long* sums; size_t slot_stride; const int* E; int n_slots; double neg2_over_n;
    int n_chunks, n_cells, dpc, d;
    float *cent, *m, *v, *grad;
    float beta1, beta2, step_size, bc2_sqrt, eps;
};
__global__ void adam_kernel(AdamLaunch a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_chunks * a.n_cells * a.dpc) return;
    const int u = idx % a.dpc, k = (idx / a.dpc) % a.n_cells, s = idx / (a.dpc * a.n_cells);
    double sum = 0.0;
    for (int c = 0; c < a.n_slots; c++) sum += (double)a.sums[(size_t)c * a.slot_stride + idx] * __builtin_ldexp(1.0, -a.E[c]);
    const float g = (float)(sum * a.neg2_over_n);
    const size_t at = (size_t)k * a.d + s * a.dpc + u;
    a.grad[at] = g;
    const float m = __fadd_rn(__fmul_rn(a.beta1, a.m[at]), __fmul_rn(__fsub_rn(1.0f, a.beta1), g));
    const float v = __fadd_rn(__fmul_rn(a.beta2, a.v[at]), __fmul_rn(__fmul_rn(__fsub_rn(1.0f, a.beta2), g), g));
    a.m[at] = m;
    a.v[at] = v;
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);
    a.cent[at] = __fsub_rn(a.cent[at], __fmul_rn(a.step_size, __fdiv_rn(m, denom)));
}

// ---- cross matrix ---------------------------------------------------------------------------------------------------------------
// M[i][s dpc + u] = sum over k ascending of ((double)sigma[s][k][i] 2^-E) (double)c[k][s dpc + u]
__global__ __launch_bounds__(256) void cross_kernel(const long long* __restrict__ sigma, const int* __restrict__ E, const float* __restrict__ cent,
                                                    int n_cells, int dpc, int d, double* __restrict__ M) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)d * d) return;
    const int i = (int)(idx % d), col = (int)(idx / d), s = col / dpc;
    const double down = __builtin_ldexp(1.0, -*E);
    const long long* sg = sigma + (size_t)s * n_cells * d + i;
    double sum = 0.0;
    for (int k = 0; k < n_cells; k++) sum += ((double)sg[(size_t)k * d] * down) * (double)cent[(size_t)k * d + col];
    M[(size_t)i * d + col] = sum;
}

__global__ void transpose_kernel(const float* __restrict__ in, int d, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)d * d) return;
    const size_t i = idx / d, j = idx % d;
    out[j * d + i] = in[idx];
}

__global__ void gather_rows_f16_kernel(const uint16_t* __restrict__ base, const uint32_t* __restrict__ ids, size_t n, int d, uint16_t* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * (size_t)d) return;
    out[idx] = base[(size_t)ids[idx / d] * d + idx % d];
}

}  // namespace

int launch_abs_max(const float* v, size_t count, uint32_t* max_bits, hipStream_t stream) {
    MSE_HIP_TRY(hipMemsetAsync(max_bits, 0, 4, stream));
    if (count == 0) return 0;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 2048);
    hipLaunchKernelGGL(abs_max_kernel, dim3(blocks), dim3(256), 0, stream, v, count, max_bits);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_fixed_exponent(const uint32_t* max_bits, size_t n, int* E, uint32_t* err, hipStream_t stream) {
    hipLaunchKernelGGL(fixed_exponent_kernel, dim3(1), dim3(1), 0, stream, max_bits, (unsigned long long)n, E, err);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_accumulate_by_code(const AccumulateArgs& g, hipStream_t stream) {
    if (g.n == 0 || g.w <= 0 || g.n_slices <= 0) return 0;
    if (g.n_cells <= 0 || g.n_cells > 256) return fail("accumulate_by_code: 1..256 cells");
    AccLaunch a;
    a.v = g.v; a.n = g.n; a.w = g.w; a.v_stride = g.v_stride; a.v_step = g.v_step;
    a.code = g.code; a.code_stride = g.code_stride; a.code_step = g.code_step;
    a.n_cells = g.n_cells; a.E = g.E;
    a.sums = reinterpret_cast<unsigned long long*>(g.sums); a.sums_step = g.sums_step;
    a.counts = g.counts;
    a.cw = g.w % 18 == 0 ? 18 : std::min(g.w, 16);     // columns per workgroup: the LDS table is n_cells x cw x 8 bytes (36 KiB at most)
    // rows per workgroup: enough that the flush (one atomic per touched cell and column) is a small part of the work, few enough
    // that a small input still spreads over the device
    a.rows_per_block = g.rows_per_block ? std::min(g.rows_per_block, 65536u) : 4096;
    const size_t bx = (g.n + a.rows_per_block - 1) / a.rows_per_block;
    if (bx > 0x7fffffffull || g.n_slices > 65535) return fail("accumulate_by_code: too many rows or slices");
    dim3 grid((unsigned)bx, (unsigned)((g.w + a.cw - 1) / a.cw), (unsigned)g.n_slices);
    const size_t lds = (size_t)a.n_cells * a.cw * 8 + (size_t)a.n_cells * 4;
    hipLaunchKernelGGL(accumulate_by_code_kernel, grid, dim3(256), lds, stream, a);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_kmeans_update(const long long* sums, const unsigned long long* counts, const int* E, int n_chunks, int n_cells, int dpc, int d,
                         float* centroids, unsigned long long* empty, hipStream_t stream) {
    const int total = n_chunks * n_cells * dpc;
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, sums, counts, E, n_chunks, n_cells, dpc, d, centroids, empty);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int residual_gemm_parts(int d) { return 2 * ((d + GN - 1) / GN); }

int launch_residual_gemm(const float* xr, const uint8_t* codes, const float* centroids, const float* Cm, size_t n, int d, int dpc, float* G,
                         float* lpart, float* lrow, hipStream_t stream) {
    if (n == 0) return 0;
    const size_t by = (n + GM - 1) / GM;
    const int n_part = residual_gemm_parts(d);
    // column blocks vary fastest: the workgroups that share 128 rows of X' run together and find them in the L2
    for (size_t y0 = 0; y0 < by; y0 += 65535) {
        const size_t my = std::min<size_t>(65535, by - y0), off = y0 * GM;
        hipLaunchKernelGGL(residual_gemm_kernel, dim3((unsigned)((d + GN - 1) / GN), (unsigned)my), dim3(256), 0, stream, xr + off * d,
                           codes + off * (size_t)(d / dpc), centroids, Cm, std::min<size_t>(n - off, my * GM), d, dpc, G ? G + off * d : nullptr,
                           lpart + off * n_part, n_part);
        MSE_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(lrow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, lpart, n_part, n, lrow);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_loss_finish(const long long* S, const int* E, size_t n, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1), 0, stream, S, E, (double)n, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_adam_step(const AdamArgs& g, hipStream_t stream) {
    AdamLaunch a;
    a.sums = g.sums; a.slot_stride = g.slot_stride; a.E = g.E; a.n_slots = g.n_slots; a.neg2_over_n = -2.0 / (double)g.n;
    a.n_chunks = g.n_chunks; a.n_cells = g.n_cells; a.dpc = g.dpc; a.d = g.d;
    a.cent = g.centroids; a.m = g.m; a.v = g.v; a.grad = g.grad;
    a.beta1 = g.beta1; a.beta2 = g.beta2; a.step_size = g.step_size; a.bc2_sqrt = g.bc2_sqrt; a.eps = g.eps;
    const int total = g.n_chunks * g.n_cells * g.dpc;
    hipLaunchKernelGGL(adam_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, a);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cross_matrix(const long long* sigma, const int* E, const float* centroids, int n_cells, int dpc, int d, double* M, hipStream_t stream) {
    const size_t total = (size_t)d * d;
    hipLaunchKernelGGL(cross_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, sigma, E, centroids, n_cells, dpc, d, M);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_transpose_f32(const float* in, int d, float* out, hipStream_t stream) {
    const size_t total = (size_t)d * d;
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, d, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_gather_rows_f16(const uint16_t* base, const uint32_t* ids, size_t n, int d, uint16_t* out, hipStream_t stream) {
    const size_t total = n * (size_t)d;
    if (total == 0) return 0;
    if ((total + 255) / 256 > 0x7fffffffull) return fail("gather_rows: too many rows");
    hipLaunchKernelGGL(gather_rows_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, base, ids, n, d, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mse
