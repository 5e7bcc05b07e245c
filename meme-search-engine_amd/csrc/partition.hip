// The shard partition on the device (include/mse.h mse_partitioner): the rows x centroids score pass of kmeans.py:78-94
// and src/dump_processor.rs:441-445, the annealing loop of kmeans.py:96-127 around it, and the sequential spill-2 walk of
// dump_processor.rs:438-461.
//
// score(x, c) = sum_k (double)x_k (double)c_k, k ascending, one f64 accumulator.  x is an f16 row, c an f32 centroid: every product has
// 11 + 24 significand bits and is exact in f64, so fma(x, c, acc) rounds exactly what acc + x c rounds.  A plain f64 VALU GEMM: one
// thread owns one row and all S <= 64 accumulators; the centroids are staged in LDS as f64, 32 k's at a time, and read as broadcasts.
#include "common.h"
#include "kernels.h"
#include "gen_ints.h"

namespace mse {
namespace {

constexpr int PT_ROWS = 256;   // rows (= threads) of a workgroup
constexpr int PT_KC = 32;      // k's of the centroids staged per step

template <int NS>
__global__ __launch_bounds__(PT_ROWS) void partition_score_kernel(PartitionScoreArgs a) {
    __shared__ __attribute__((aligned(16))) double cs[PT_KC][NS];
    __shared__ unsigned hist[2 * 64];
    if (a.stopped && *a.stopped) return;
    const int tid = threadIdx.x, S = a.S, d = a.d;
    if (tid < 2 * 64) hist[tid] = 0u;
    const size_t r = (size_t)blockIdx.x * PT_ROWS + tid;
    const bool live = r < a.n;
    const size_t rr = live ? r : a.n - 1;                       // the ragged tail computes the last row again and writes nothing
    const size_t src = a.ids ? (size_t)a.ids[rr] : rr;
    const uint4* row = reinterpret_cast<const uint4*>(a.rows + src * (size_t)d);
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = 0.0;
    for (int k0 = 0; k0 < d; k0 += PT_KC) {
        __syncthreads();                                         // the previous step's reads are done (first pass: hist is zeroed)
        for (int e = tid; e < PT_KC * NS; e += PT_ROWS) {
            const int s = e / PT_KC, kk = e % PT_KC;
            cs[kk][s] = (s < S && k0 + kk < d) ? (double)a.cen[(size_t)s * d + k0 + kk] : 0.0;
        }
        __syncthreads();
        const int kn = d - k0 < PT_KC ? d - k0 : PT_KC;          // a multiple of 8
        for (int k8 = 0; k8 < kn; k8 += 8) {
            const uint4 v = row[(k0 + k8) >> 3];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint16_t h = (uint16_t)(w[j >> 1] >> ((j & 1) * 16));
                const double x = (double)(float)__builtin_bit_cast(_Float16, h);
                const double* c = cs[k8 + j];
#pragma unroll
                for (int s = 0; s < NS; s++) acc[s] = __builtin_fma(x, c[s], acc[s]);
            }
        }
    }
    // the row's two best centroids: f64 score descending, lowest index on ties
    int i1 = 0, i2 = 1;
    double v1 = -__builtin_inf(), v2 = -__builtin_inf();
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < S) {
            const double v = acc[s];
            if (v > v1) { v2 = v1; i2 = i1; v1 = v; i1 = s; }
            else if (v > v2) { v2 = v; i2 = s; }
        }
    }
    if (i2 == i1) i2 = i1 == 0 ? 1 : 0;                          // (only a row without one finite score gets here)
    if (live) {
        if (a.top2) { a.top2[r * 2] = (uint8_t)i1; a.top2[r * 2 + 1] = (uint8_t)i2; }
        if (a.scores) {
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (s < S) a.scores[r * (size_t)S + s] = acc[s];
        }
        if (a.sizes) { atomicAdd(&hist[i1], 1u); atomicAdd(&hist[64 + i2], 1u); }
    }
    if (a.sizes) {
        __syncthreads();
        if (tid < 2 * 64) {
            const int rank = tid >> 6, s = tid & 63;
            if (s < S && hist[tid]) atomicAdd(&a.sizes[rank * S + s], (unsigned long long)hist[tid]);
        }
    }
}

// z(key)[j] = (float)ints(seed, key)[j] * K, K = (float)(sqrt(3) / 65536): unit variance, bounded at +-3.47
__device__ __forceinline__ float noise_scale() { return (float)(1.7320508075688772 / 65536.0); }
__device__ __forceinline__ void noise_pair(uint32_t seed, uint64_t key, uint32_t call, float& a, float& b) {
    int ia, ib;
    pair_of(seed, key, call, ia, ib);
    a = __fmul_rn((float)ia, noise_scale());
    b = __fmul_rn((float)ib, noise_scale());
}

// norm of the row v (d floats, visible to the whole workgroup): ss = sum of (double)v_k^2, k ascending, by ONE thread; sqrt by 48 Newton
// steps from 1 (+ * / only, as gen.hip: the same bits on any IEEE machine).  0 for a zero row.  Every thread gets the value
__device__ double row_norm_seq(const float* v, int d, double* slot) {
    if (threadIdx.x == 0) {
        double ss = 0.0;
        for (int k = 0; k < d; k++) { const double x = (double)v[k]; ss = ss + x * x; }
        double y = 0.0;
        if (ss > 0.0) {
            y = 1.0;
#pragma unroll 1
            for (int i = 0; i < 48; i++) y = 0.5 * (y + ss / y);
        }
        *slot = y;
    }
    __syncthreads();
    return *slot;
}

// one workgroup per centroid
__global__ __launch_bounds__(256) void partition_candidate_kernel(PartitionAnnealArgs a) {
    __shared__ double slot;
    const PartitionDevState st = *a.st;
    if (st.stopped) return;
    const int s = blockIdx.x, d = a.d;
    const float* cur = a.c[st.cur & 1u] + (size_t)s * d;
    float* cand = a.c[(st.cur & 1u) ^ 1u] + (size_t)s * d;
    const uint64_t key = st.t * (uint64_t)a.S + (uint64_t)s;
    for (int c = threadIdx.x; c < d / 2; c += blockDim.x) {
        float za, zb;
        noise_pair(a.seed, key, (uint32_t)c, za, zb);
        if (st.t != 0) {
            za = __fadd_rn(cur[2 * c], __fmul_rn(za, st.T));
            zb = __fadd_rn(cur[2 * c + 1], __fmul_rn(zb, st.T));
        }
        cand[2 * c] = za;
        cand[2 * c + 1] = zb;
    }
    __syncthreads();
    const double norm = row_norm_seq(cand, d, &slot);
    float* out = a.nrm + (size_t)s * d;
    for (int k = threadIdx.x; k < d; k += blockDim.x) out[k] = norm > 0.0 ? (float)((double)cand[k] / norm) : cand[k];
}

__global__ __launch_bounds__(256) void partition_normalise_kernel(const float* __restrict__ c, int d, float* __restrict__ out,
                                                                  uint16_t* __restrict__ f16_out, float* __restrict__ wide_out) {
    __shared__ double slot;
    const int s = blockIdx.x;
    const float* v = c + (size_t)s * d;
    const double norm = row_norm_seq(v, d, &slot);
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        const float x = norm > 0.0 ? (float)((double)v[k] / norm) : v[k];
        out[(size_t)s * d + k] = x;
        const _Float16 h = (_Float16)x;
        if (f16_out) f16_out[(size_t)s * d + k] = __builtin_bit_cast(uint16_t, h);
        if (wide_out) wide_out[(size_t)s * d + k] = (float)h;
    }
}

__global__ void partition_noise_kernel(uint32_t seed, uint64_t key, int d, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d / 2) return;
    noise_pair(seed, key, (uint32_t)c, out[2 * c], out[2 * c + 1]);
}

// The decision is one thread's; the rest of the workgroup only zeroes the histogram and rewrites the rerolled rows
__global__ __launch_bounds__(256) void partition_decide_kernel(PartitionAnnealArgs a) {
    __shared__ int reroll[3];   // flag, worst[0], worst[1]
    __shared__ unsigned long long sh_t;
    __shared__ uint32_t sh_cur;
    if (a.st->stopped) return;
    const int S = a.S;
    if (threadIdx.x == 0) {
        PartitionDevState st = *a.st;
        unsigned long long F = 0;
        int worst[2] = {0, 0};
        for (int rank = 0; rank < 2; rank++) {
            unsigned long long wmax = 0;
            for (int s = 0; s < S; s++) {
                const long long diff = (long long)((unsigned long long)S * a.sizes[rank * S + s]) - (long long)a.n;
                const unsigned long long v = (unsigned long long)(diff < 0 ? -diff : diff);
                if (v > wmax) { wmax = v; worst[rank] = s; }    // the first index that attains the maximum
            }
            if (wmax > F) F = wmax;
        }
        reroll[0] = 0;
        sh_t = st.t;
        if (st.t == 0) {                                         // the initial evaluation (kmeans.py:100)
            st.last = F; st.li = 0; st.cur ^= 1u;
        } else {
            uint8_t code = 0;
            if (F < st.last) { st.cur ^= 1u; st.T = __fmul_rn(st.T, a.accept_decay); st.last = F; st.li = 0; code = 1; }
            else { st.T = __fmul_rn(st.T, a.reject_decay); st.li += 1; }
            if (st.li > (unsigned long long)a.reroll_after) {    // (:114-119; last takes the CANDIDATE's fitness: the script's quirk)
                st.li = 0; st.T = __fmul_rn(st.T, a.reroll_heat); st.last = F; code = 2;
                reroll[0] = 1; reroll[1] = worst[0]; reroll[2] = worst[1];
            }
            if (st.last * a.stop_den < (unsigned long long)a.n * a.stop_num) st.stopped = 1u;   // (:120-121: before the cap)
            else st.T = st.T < a.cap ? st.T : a.cap;
            if (st.t - 1 < a.trace_cap) { a.trace_F[st.t - 1] = F; a.trace_code[st.t - 1] = code; }
        }
        st.t += 1;
        sh_cur = st.cur & 1u;
        *a.st = st;
    }
    __syncthreads();
    if (threadIdx.x < 2 * S) a.sizes[threadIdx.x] = 0ull;
    if (reroll[0]) {
        for (int w = 1; w <= 2; w++) {
            const int s = reroll[w];
            float* row = a.c[sh_cur] + (size_t)s * a.d;
            const uint64_t key = ((uint64_t)1 << 40) + sh_t * (uint64_t)S + (uint64_t)s;
            for (int c = threadIdx.x; c < a.d / 2; c += blockDim.x) noise_pair(a.seed, key, (uint32_t)c, row[2 * c], row[2 * c + 1]);
        }
    }
}

struct Cand { long long key; int idx; };
__device__ __forceinline__ bool cand_less(const Cand& a, const Cand& b) { return a.key < b.key || (a.key == b.key && a.idx < b.idx); }

// One wave, lane = shard.  Per row every lane forms its key; a six-step butterfly merges the two smallest (key, shard) pairs of the
// wave, so every lane knows both choices.  The next row's score is in flight during the merge
__global__ __launch_bounds__(64) void partition_walk_kernel(const double* __restrict__ scores, size_t rows, int S, double fudge,
                                                            unsigned long long* __restrict__ counts, unsigned long long* __restrict__ bal,
                                                            uint8_t* __restrict__ assignment) {
    const int lane = threadIdx.x;
    const bool mine = lane < S;
    unsigned long long cnt = mine ? counts[lane] : 0ull, b = *bal;
    double nxt = mine && rows ? scores[lane] : 0.0;
    for (size_t i = 0; i < rows; i++) {
        const double sc = nxt;
        if (mine && i + 1 < rows) nxt = scores[(i + 1) * (size_t)S + lane];
        Cand lo{INT64_MAX, 64 + lane}, hi{INT64_MAX, 255};
        if (mine) {
            const double adj = sc - fudge * ((double)cnt / (double)b);
            lo.key = (long long)(0ull - (unsigned long long)scale_dot_result_f64(adj));
            lo.idx = lane;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            Cand plo, phi;
            plo.key = __shfl_xor(lo.key, o); plo.idx = __shfl_xor(lo.idx, o);
            phi.key = __shfl_xor(hi.key, o); phi.idx = __shfl_xor(hi.idx, o);
            if (cand_less(plo, lo)) { hi = cand_less(lo, phi) ? lo : phi; lo = plo; }
            else if (cand_less(plo, hi)) hi = plo;
        }
        if (lane == lo.idx || lane == hi.idx) cnt += 1;
        b += 1;
        if (lane == 0) { assignment[i * 2] = (uint8_t)lo.idx; assignment[i * 2 + 1] = (uint8_t)hi.idx; }
    }
    if (mine) counts[lane] = cnt;
    if (lane == 0) *bal = b;
}

__global__ __launch_bounds__(256) void partition_shard_bits_kernel(const uint8_t* __restrict__ assignment, size_t n, int s,
                                                                   uint32_t* __restrict__ bits) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool hit = r < n && (assignment[r * 2] == s || assignment[r * 2 + 1] == s);
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && (r & ~(size_t)63) < n) {
        bits[(r >> 6) * 2] = (uint32_t)m;
        bits[(r >> 6) * 2 + 1] = (uint32_t)(m >> 32);
    }
}

}  // namespace

int launch_partition_score(const PartitionScoreArgs& a, hipStream_t stream) {
    if (a.n == 0) return 0;
    if (a.S < 2 || a.S > 64 || a.d <= 0 || a.d % 8) return fail("partition: 2 .. 64 shards and a width that is a multiple of 8");
    const dim3 grid((unsigned)((a.n + PT_ROWS - 1) / PT_ROWS)), block(PT_ROWS);
    if (a.S <= 8) hipLaunchKernelGGL(partition_score_kernel<8>, grid, block, 0, stream, a);
    else if (a.S <= 16) hipLaunchKernelGGL(partition_score_kernel<16>, grid, block, 0, stream, a);
    else if (a.S <= 32) hipLaunchKernelGGL(partition_score_kernel<32>, grid, block, 0, stream, a);
    else if (a.S <= 48) hipLaunchKernelGGL(partition_score_kernel<48>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(partition_score_kernel<64>, grid, block, 0, stream, a);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_partition_candidate(const PartitionAnnealArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(partition_candidate_kernel, dim3((unsigned)a.S), dim3(256), 0, stream, a);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_partition_decide(const PartitionAnnealArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(partition_decide_kernel, dim3(1), dim3(256), 0, stream, a);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_partition_normalise(const float* c, int S, int d, float* out, uint16_t* f16_out, float* wide_out, hipStream_t stream) {
    hipLaunchKernelGGL(partition_normalise_kernel, dim3((unsigned)S), dim3(256), 0, stream, c, d, out, f16_out, wide_out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_partition_noise(uint32_t seed, uint64_t key, int d, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(partition_noise_kernel, dim3((unsigned)((d / 2 + 255) / 256)), dim3(256), 0, stream, seed, key, d, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_partition_walk(const double* scores, size_t rows, int S, double fudge, unsigned long long* counts, unsigned long long* bal,
                          uint8_t* assignment, hipStream_t stream) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(partition_walk_kernel, dim3(1), dim3(64), 0, stream, scores, rows, S, fudge, counts, bal, assignment);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_partition_shard_bits(const uint8_t* assignment, size_t n, int s, uint32_t* bits, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(partition_shard_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, assignment, n, s, bits);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mse
