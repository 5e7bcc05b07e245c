// Descriptor bytes of a resident index (the last host-in / host-out stage of dump_processor's packer):
//
//   score_mlp_kernel       src/score_model.rs:13-32 over the base's f16 rows: down . silu(up . x + bias) * d_emb / d_hidden, fused -- the
//                          [rows][d_hidden] activations live in registers only
//   select_count_kernel /  meme-rater/compute_cdf.py:64-71 needs order statistics of every channel: exact multi-rank radix select, three
//   select_resolve_kernel  histogram passes (11 / 11 / 10 bits), integer atomics only
//   describe_kernel        src/dump_processor.rs:481-491: bucket(cdf_j, value_j) into the resident codes' descriptor bytes
//
// THE SUMMATION ORDERS of the score (tests/describe_ref.py restates them; bit for bit wherever silu is saturated):
//   pre-activation  s = fma(up[n][K-1], x[K-1], ... fma(up[n][0], x[0], +0)): v_mfma_f32_32x32x2_f32 is a k-ordered f32 fma chain and one wave
//                   feeds one output its k pairs in ascending order.  k past d_emb is fed as 0 * 0, which leaves the bits as they are
//   bias            s = s + bias[n], one f32 add
//   silu            h = s / (1 + expf(-s))        (as dense_rows_kernel of index_pack.hip writes it)
//   hidden sum      the hidden units are walked in tiles of 128, a tile in two halves of 64 (w = 0, 1).  Per output channel c, for the
//                   half (tile t, w) with units n_j = 128 t + 64 w + j:
//                       u_j = fma(h[n_{j+32}], down[c][n_{j+32}], h[n_j] * down[c][n_j])            j < 32  (units past d_hidden give +0)
//                       S   = the xor butterfly over u_0 .. u_31: five rounds v_j = v_j + v_{j ^ o}, o = 1, 2, 4, 8, 16
//                       T_w = T_w + S                                                            t ascending, from +0
//                   and at the end score = (T_0 + T_1) * (f32(d_emb) / f32(d_hidden)).
// None of this names the row's place in its tile, the number of rows of the call, ids versus range, or the grid: a row's score bits are the
// same however it is asked for (one workgroup owns a tile of 128 rows and walks all hidden tiles itself; no atomics).
//
// Tile: 128 rows x 128 hidden units per step, k in steps of 32 through LDS (34 KB), four waves of 2 x 2 MFMA tiles -- residual_gemm_kernel's
// shape (pq_train.hip), with B read as up[n][k] (the safetensors layout: no transposed copy is kept) and A widened from f16 as it is loaded;
// a thread loads 16 consecutive k of one row and of one hidden unit per step, 16 bytes at a time where the width is a multiple of 8.
#include "describe.h"
#include "index_pack.h"

namespace mse {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr int DM = 128, DN = 128, DK = 32;
constexpr int D_LS = DK + 1;          // [row or unit][k], odd stride: the 32 rows of a half-wave land in 32 banks
constexpr int MAX_CH = 8;

// the five rounds of the butterfly over the 32 lanes of a half-wave without a trip through LDS for the first four: quad permutes are
// j ^ 1 and j ^ 2; after them the four lanes of a quad are equal, so the mirrored lane of the 8 (of the 16) holds what lane j ^ 4 (j ^ 8)
// holds and row_half_mirror / row_mirror stand in for the xor; the last round is a swizzle by 16
template <int CTRL>
__device__ __forceinline__ float add_dpp(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false);
    return __fadd_rn(v, __builtin_bit_cast(float, o));
}
__device__ __forceinline__ float butterfly32(float v) {
    v = add_dpp<0xB1>(v);      // quad_perm [1, 0, 3, 2]
    v = add_dpp<0x4E>(v);      // quad_perm [2, 3, 0, 1]
    v = add_dpp<0x141>(v);     // row_half_mirror
    v = add_dpp<0x140>(v);     // row_mirror
    const int o = __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F);   // bit mode: and 0x1F, or 0, xor 0x10
    return __fadd_rn(v, __builtin_bit_cast(float, o));
}

__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) {
    return (float)__builtin_bit_cast(_Float16, h);   // exact widening (half::f16::to_f32)
}

__global__ __launch_bounds__(256, 2) void score_mlp_kernel(const uint16_t* __restrict__ rows, int d, const uint32_t* __restrict__ ids, size_t first,
                                                           size_t n, const float* __restrict__ up, const float* __restrict__ bias,
                                                           const float* __restrict__ down, int d_hidden, int out_ch, float scale,
                                                           int vec, float* __restrict__ scores) {
    __shared__ float As[DM * D_LS];
    __shared__ float Bs[DN * D_LS];
    __shared__ unsigned long long src[DM];   // base row of each tile row, ~0 past the end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const size_t i0 = (size_t)blockIdx.x * DM;
    if (tid < DM) {
        const size_t gi = i0 + tid;
        src[tid] = gi < n ? (ids ? (unsigned long long)ids[gi] : (unsigned long long)(first + gi)) : ~0ull;
    }
    __syncthreads();
    // a thread fetches 16 consecutive k of ONE tile row and of ONE hidden unit per k step: one base pointer each, set once per tile, and --
    // where the width allows it (vec: d a multiple of 8 and 16-byte aligned bases) -- 16-byte loads
    const int fr = tid >> 1, fk = (tid & 1) * 16;
    const uint16_t* const ap = src[fr] != ~0ull ? rows + (size_t)src[fr] * d : nullptr;
    const float* bp = nullptr;
    float tot[MAX_CH];
#pragma unroll
    for (int c = 0; c < MAX_CH; c++) tot[c] = 0.0f;
    float ra[16], rb[16];
    auto fetch = [&](int k0) {
        const int k = k0 + fk;
        if (vec && k + 16 <= d) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                h8 v;
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] = (_Float16)0.0f;
                if (ap) v = *reinterpret_cast<const h8*>(ap + k + 8 * q);
#pragma unroll
                for (int j = 0; j < 8; j++) ra[8 * q + j] = (float)v[j];   // exact widening (half::f16::to_f32)
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (bp) v = *reinterpret_cast<const f32x4*>(bp + k + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; j++) rb[4 * q + j] = v[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                ra[j] = (ap && k + j < d) ? f16_bits_to_f32(ap[k + j]) : 0.0f;
                rb[j] = (bp && k + j < d) ? bp[k + j] : 0.0f;
            }
        }
    };
    for (int n0 = 0; n0 < d_hidden; n0 += DN) {
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
        bp = n0 + fr < d_hidden ? up + (size_t)(n0 + fr) * d : nullptr;
        fetch(0);
        for (int k0 = 0; k0 < d; k0 += DK) {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                As[fr * D_LS + fk + j] = ra[j];
                Bs[fr * D_LS + fk + j] = rb[j];
            }
            __syncthreads();
            if (k0 + DK < d) fetch(k0 + DK);
#pragma unroll
            for (int t = 0; t < DK / 2; t++) {
                const float a0 = As[(wm * 64 + l31) * D_LS + 2 * t + lh];
                const float a1 = As[(wm * 64 + 32 + l31) * D_LS + 2 * t + lh];
                const float b0 = Bs[(wn * 64 + l31) * D_LS + 2 * t + lh];
                const float b1 = Bs[(wn * 64 + 32 + l31) * D_LS + 2 * t + lh];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            __syncthreads();
        }
        // epilogue in registers: this lane's two hidden units are n0 + 64 wn + l31 and that + 32
        const int c0 = n0 + wn * 64 + l31, c1 = c0 + 32;
        const bool in0 = c0 < d_hidden, in1 = c1 < d_hidden;
        const float bias0 = in0 ? bias[c0] : 0.0f, bias1 = in1 ? bias[c1] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float s0 = __fadd_rn(acc[mt][0][r], bias0), s1 = __fadd_rn(acc[mt][1][r], bias1);
                s0 = s0 / (1.0f + expf(-s0));
                s1 = s1 / (1.0f + expf(-s1));
                acc[mt][0][r] = in0 ? s0 : 0.0f;
                acc[mt][1][r] = in1 ? s1 : 0.0f;
            }
#pragma unroll
        for (int c = 0; c < MAX_CH; c++) {
            if (c < out_ch) {
                const float d0 = in0 ? down[(size_t)c * d_hidden + c0] : 0.0f, d1 = in1 ? down[(size_t)c * d_hidden + c1] : 0.0f;
                float mine = 0.0f;   // S of the tile row whose slot (16 mt + r) is this lane's l31
#pragma unroll
                for (int mt = 0; mt < 2; mt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float v = butterfly32(fmaf(acc[mt][1][r], d1, __fmul_rn(acc[mt][0][r], d0)));
                        if (l31 == 16 * mt + r) mine = v;
                    }
                tot[c] = __fadd_rn(tot[c], mine);
            }
        }
    }
    // lane (lh, l31) of wave (wm, wn) holds T_wn of tile row wm 64 + 32 mt + (r & 3) + 8 (r >> 2) + 4 lh with 16 mt + r = l31
    float* xch = As;                         // [c][wm][lane]; the last k step's barrier has passed
    if (wn == 1) {
#pragma unroll
        for (int c = 0; c < MAX_CH; c++)
            if (c < out_ch) xch[(c * 2 + wm) * 64 + lane] = tot[c];
    }
    __syncthreads();
    if (wn == 0) {
        const int mt = l31 >> 4, r = l31 & 15;
        const size_t gi = i0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gi < n) {
#pragma unroll
            for (int c = 0; c < MAX_CH; c++)
                if (c < out_ch) scores[gi * out_ch + c] = __fmul_rn(__fadd_rn(tot[c], xch[(c * 2 + wm) * 64 + lane]), scale);
        }
    }
}

// ---- multi-rank radix select ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t select_key(uint32_t bits, int as_f32) {
    if (!as_f32) return bits;
    if (bits == 0x80000000u) bits = 0;                       // -0.0 sorts with +0.0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

template <int PASS>
__global__ __launch_bounds__(256) void select_count_kernel(const uint32_t* __restrict__ data, size_t stride, size_t n, int as_f32,
                                                           uint32_t* __restrict__ cnt, uint32_t* __restrict__ n_nan,
                                                           const uint16_t* __restrict__ slot1, const uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ n_slots) {
    __shared__ uint32_t hist[PASS == 1 ? SEL_BINS12 : 1];
    __shared__ uint16_t s1[PASS == 1 ? 1 : SEL_BINS12];
    __shared__ uint32_t sp[PASS == 3 ? SEL_MAX_RANKS : 1];
    const int tid = threadIdx.x;
    int ns = 0;
    if (PASS == 1) {
        for (int i = tid; i < SEL_BINS12; i += 256) hist[i] = 0;
    } else {
        for (int i = tid; i < SEL_BINS12; i += 256) s1[i] = slot1[i];
        if (PASS == 3) {
            ns = (int)*n_slots;
            if (ns > SEL_MAX_RANKS) ns = SEL_MAX_RANKS;
            for (int i = tid; i < ns; i += 256) sp[i] = sorted[i];
        }
    }
    __syncthreads();
    uint32_t nan_seen = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t bits = data[i * stride];
        if (PASS == 1 && as_f32 && (bits & 0x7FFFFFFFu) > 0x7F800000u) { nan_seen++; continue; }
        const uint32_t key = select_key(bits, as_f32);
        if (PASS == 1) {
            atomicAdd(&hist[key >> 21], 1u);
        } else {
            const uint32_t s = s1[key >> 21];
            if (s == SEL_NO_SLOT) continue;
            if (PASS == 2) {
                atomicAdd(&cnt[(size_t)s * SEL_BINS12 + ((key >> 10) & (SEL_BINS12 - 1))], 1u);
            } else {
                const uint32_t p = key >> 10;
                int lo = 0, hi = ns;                         // first slot whose prefix is >= p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sp[mid] < p) lo = mid + 1; else hi = mid;
                }
                if (lo < ns && sp[lo] == p) atomicAdd(&cnt[(size_t)lo * SEL_BINS3 + (key & (SEL_BINS3 - 1))], 1u);
            }
        }
    }
    if (PASS == 1) {
        if (nan_seen) atomicAdd(n_nan, nan_seen);
        __syncthreads();
        for (int i = tid; i < SEL_BINS12; i += 256)
            if (hist[i]) atomicAdd(&cnt[i], hist[i]);
    }
}

// one workgroup of 512 threads.  Part 1, a wave per rank: find the bin of the rank's counter row that holds it.  Part 2, a thread per
// rank: number the distinct new prefixes in ascending order -- that number is the prefix's counter row in the next pass
template <int LEVEL>
__global__ __launch_bounds__(512) void select_resolve_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ rem, uint32_t* __restrict__ prefix,
                                                             uint32_t* __restrict__ slot, uint32_t* __restrict__ sorted,
                                                             uint32_t* __restrict__ n_slots, uint16_t* __restrict__ slot1, int nr) {
    constexpr int BINS = LEVEL == 3 ? SEL_BINS3 : SEL_BINS12, BITS = LEVEL == 3 ? 10 : 11, PER = BINS / 64;
    __shared__ uint32_t pf[SEL_MAX_RANKS];
    __shared__ uint32_t lead[SEL_MAX_RANKS];
    __shared__ uint32_t n_lead;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) n_lead = 0;
    for (int i = wave; i < nr; i += 8) {
        const uint32_t* seg = LEVEL == 1 ? cnt : cnt + (size_t)slot[i] * BINS;
        const uint32_t r = rem[i];
        uint32_t sum = 0;
        for (int t = 0; t < PER; t++) sum += seg[lane * PER + t];
        uint32_t incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const uint32_t excl = incl - sum;
        bool hit = r >= excl && r < incl;
        if (!__any(hit)) hit = lane == 63;                   // a rank past the count cannot happen (the host checks ranks < n)
        if (hit) {
            uint32_t run = excl;
            int digit = lane * PER + PER - 1;
            uint32_t left = 0;
            for (int t = 0; t < PER; t++) {
                const uint32_t c = seg[lane * PER + t];
                if (r - run < c) { digit = lane * PER + t; left = r - run; break; }
                run += c;
            }
            pf[i] = ((LEVEL == 1 ? 0u : prefix[i]) << BITS) | (uint32_t)digit;
            rem[i] = left;
        }
    }
    if (LEVEL == 1)
        for (int i = tid; i < SEL_BINS12; i += 512) slot1[i] = (uint16_t)SEL_NO_SLOT;
    __syncthreads();
    if (tid < nr) {
        const uint32_t p = pf[tid];
        bool first = true;
        for (int j = 0; j < tid; j++) first = first && pf[j] != p;
        lead[tid] = first;
    }
    __syncthreads();
    if (tid < nr) {
        const uint32_t p = pf[tid];
        uint32_t less = 0;
        for (int j = 0; j < nr; j++) less += (lead[j] && pf[j] < p) ? 1u : 0u;
        prefix[tid] = p;
        slot[tid] = less;
        if (lead[tid]) {
            sorted[less] = p;
            atomicAdd(&n_lead, 1u);
            if (LEVEL == 1) slot1[p] = (uint16_t)less;
        }
    }
    __syncthreads();
    if (tid == 0) *n_slots = n_lead;
}

__global__ __launch_bounds__(256) void describe_kernel(const float* __restrict__ cdfs, int cdf_len, const float* __restrict__ scores, int n_ch,
                                                       const uint32_t* __restrict__ ts, const uint32_t* __restrict__ ids, size_t first, size_t n,
                                                       uint8_t* __restrict__ desc, int n_desc) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * (size_t)n_desc) return;
    const size_t i = idx / n_desc;
    const int j = (int)(idx % n_desc);
    const float v = j < n_ch ? scores[i * n_ch + j] : (float)ts[i];   // dump_processor.rs:481 `as f32`: round to nearest
    const size_t row = ids ? (size_t)ids[i] : first + i;
    desc[row * n_desc + j] = descriptor_bucket(cdfs + (size_t)j * cdf_len, cdf_len, v);
}

}  // namespace

SelectScratch select_scratch_at(uint32_t* base) {
    SelectScratch s;
    s.cnt1 = base;
    s.cnt2 = s.cnt1 + SEL_BINS12;
    s.cnt3 = s.cnt2 + (size_t)SEL_MAX_RANKS * SEL_BINS12;
    s.n_nan = s.cnt3 + (size_t)SEL_MAX_RANKS * SEL_BINS3;
    s.rem = s.n_nan + 1;
    s.prefix = s.rem + SEL_MAX_RANKS;
    s.slot = s.prefix + SEL_MAX_RANKS;
    s.sorted = s.slot + SEL_MAX_RANKS;
    s.n_slots = s.sorted + SEL_MAX_RANKS;
    s.slot1 = reinterpret_cast<uint16_t*>(s.n_slots + 1);
    return s;
}

void launch_score_mlp(const uint16_t* rows, int d, const uint32_t* ids, size_t first, size_t n, const float* up, const float* bias,
                      const float* down, int d_hidden, int out_ch, float* scores, hipStream_t st) {
    const float scale = (float)d / (float)d_hidden;   // score_model.rs:16
    const int vec = d % 8 == 0 && (((uintptr_t)rows | (uintptr_t)up) & 15) == 0;   // every row and weight row starts 16-byte aligned
    hipLaunchKernelGGL(score_mlp_kernel, dim3((unsigned)((n + DM - 1) / DM)), dim3(256), 0, st, rows, d, ids, first, n, up, bias, down, d_hidden,
                       out_ch, scale, vec, scores);
}

void launch_select_count(int pass, const uint32_t* data, size_t stride, size_t n, int as_f32, const SelectScratch& sc, hipStream_t st) {
    size_t blocks = (n + 4095) / 4096;
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    const dim3 g((unsigned)blocks), b(256);
    if (pass == 1)
        hipLaunchKernelGGL(select_count_kernel<1>, g, b, 0, st, data, stride, n, as_f32, sc.cnt1, sc.n_nan, sc.slot1, sc.sorted, sc.n_slots);
    else if (pass == 2)
        hipLaunchKernelGGL(select_count_kernel<2>, g, b, 0, st, data, stride, n, as_f32, sc.cnt2, sc.n_nan, sc.slot1, sc.sorted, sc.n_slots);
    else
        hipLaunchKernelGGL(select_count_kernel<3>, g, b, 0, st, data, stride, n, as_f32, sc.cnt3, sc.n_nan, sc.slot1, sc.sorted, sc.n_slots);
}

void launch_select_resolve(int level, const SelectScratch& sc, int n_ranks, hipStream_t st) {
    if (level == 1)
        hipLaunchKernelGGL(select_resolve_kernel<1>, dim3(1), dim3(512), 0, st, sc.cnt1, sc.rem, sc.prefix, sc.slot, sc.sorted, sc.n_slots, sc.slot1, n_ranks);
    else if (level == 2)
        hipLaunchKernelGGL(select_resolve_kernel<2>, dim3(1), dim3(512), 0, st, sc.cnt2, sc.rem, sc.prefix, sc.slot, sc.sorted, sc.n_slots, sc.slot1, n_ranks);
    else
        hipLaunchKernelGGL(select_resolve_kernel<3>, dim3(1), dim3(512), 0, st, sc.cnt3, sc.rem, sc.prefix, sc.slot, sc.sorted, sc.n_slots, sc.slot1, n_ranks);
}

void launch_describe(const float* cdfs, int cdf_len, const float* scores, int n_ch, const uint32_t* ts, const uint32_t* ids, size_t first,
                     size_t n, uint8_t* desc, int n_desc, hipStream_t st) {
    const size_t total = n * (size_t)n_desc;
    hipLaunchKernelGGL(describe_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cdfs, cdf_len, scores, n_ch, ts, ids, first, n, desc,
                       n_desc);
}

}  // namespace mse
