// The ensemble rater of the reference's meme-rater/ on the device (model.py: M one-hidden-layer MLPs under a Bradley-Terry head;
// train.py:63-71: binary cross-entropy on the win probabilities, backward, torch.optim.AdamW; active_learning.py:53: the variance of the
// members' win probabilities), over the wide layout of ensemble_to_wide_model.py:44-55.
//
//   rater_forward_kernel        u = up . x + bias and h = silu(u) of every (member, slot, unit) on the f32 matrix cores
//   rater_scores_kernel         s = down . h, one wave per (member, slot)
//   rater_check_rows_kernel     a non-finite row in a slot of the step
//   rater_head_kernel           z, p, the gradient g of every (member, pair, channel), the loss and the gate
//   rater_du_kernel             the hidden gradient through silu
//   rater_down_kernel           down's gradient and update;  rater_bias_kernel: bias's
//   rater_update_kernel         ONE pass over up and its two moment arrays: an element's gradient is formed on the fly from the step's
//                               du and x; no [M E][E] gradient exists
//   rater_pair_variance_kernel  a thread per candidate pair over a member-score table
//
// THE RULE (tests/rater_ref.py restates it; bit for bit).  M members, E = d_emb, C channels, B pairs per member and step, R = 2 B slots:
// slot 2 b is pair b's first row, slot 2 b + 1 its second; member m owns hidden units m E .. (m + 1) E of the f32 parameters
// up [M E][E], bias [M E], down [C][M E]; every parameter with moments m and v of its shape; one step count t.  x[m][r] is the exact
// widening of the f16 row in slot r of member m.
//   exp_fixed   rater_math.h; sig, silu and silu' derive from it there, each in one stated operation order
//   forward     u[m][r][j] = A + bias[m E + j], one f32 add, A = fma(up[m E + j][E-1], x[E-1], ... fma(up[m E + j][0], x[0], +0)): the
//               k-ascending chain of describe.hip (v_mfma_f32_32x32x2_f32 is one);  h = silu(u)
//   scores      s[m][r][c]: 64 lanes, lane l the chain S_l = fma(h[j], down[c][m E + j], S_l) over j = l, l + 64, ... ascending from +0 (a
//               lane without a j holds +0), then the tree S_l = S_l + S_{l + o}, o = 32, 16, ..., 1, l < o; s = S_0
//   head        z = s[m][2b][c] - s[m][2b+1][c]; p = sig(z); g[m][b][c] = (p - y) * invN, invN = (float)(1.0 / (double)(M B C)) from the
//               host.  (The mean-reduced BCE of train.py:66-67 through the sigmoid in closed form; where p rounds to 0 or 1 torch's
//               clamped log and its p (1 - p) factor give 0 and this rule keeps (p - y) / N.)
//   loss        reported only: per element -(y lp + (1 - y) lq) in f64 with lp = log(p), lq = log(1 - p) from the f32 p, each raised to
//               -100 where below; summed over (m, b, c) ascending from +0, divided by (double)(M B C)
//   gate        a step with a non-finite row in a slot or a non-finite loss is refused: weights, moments and t stay, later steps of the
//               call are not run
//   backward    with the weights from before the update; ds[r][c] = g[m][r / 2][c], negated for odd r:
//               g_down[c][m E + j] = fma(ds[r][c], h[m][r][j], G) over r ascending from +0
//               dh[r][j] = fma(ds[r][c], down[c][m E + j], D) over c ascending from +0;  du[m][r][j] = dh * silu'(u[m][r][j])
//               g_bias[m E + j] = G + du[m][r][j] over r ascending from +0
//               g_up[m E + j][k] = fma(du[m][r][j], x[m][r][k], G) over r ascending from +0
//   AdamW       sae_train.hip's, unchanged: p = p * decay; m = beta1 m + (1 - beta1) g; v = beta2 v + ((1 - beta2) g) g;
//               p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps)), every operation rounded once, sqrtf and the quotients correctly;
//               the per-step constants in double on the host.  Every parameter moves at every step
//   variance    per pair (a, b) of table rows and channel c: p_m = sig(s[a][m][c] - s[b][m][c]); mean = (p_0 + ... + p_{M-1}, m ascending
//               from +0) / (float)M; var = ((p_m - mean)^2 summed the same way, square then add) / (float)(M - 1); the result is the
//               largest var over c (v > best ? v : best, c ascending from channel 0's)
// Nothing in it names the grid, a tile, the row's place in a call, ids versus host rows or how a run is cut into calls.
//
// Forward tile: score_mlp_kernel's (describe.hip) -- 128 slots x 128 hidden units, k in steps of 32 through LDS, four waves of 2 x 2
// MFMA tiles -- with one workgroup per (slot tile, unit tile of ONE member, member): a member's units are walked from its own first
// unit, so members need not fall on tile boundaries, and units past E are guarded.
#include "rater.h"
#include "rater_math.h"

namespace mse {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr int DM = 128, DN = 128, DK = 32;
constexpr int D_LS = DK + 1;          // [slot or unit][k], odd stride: the 32 rows of a half-wave land in 32 banks
constexpr int MAX_CH = (int)RATER_MAX_CHANNELS;

__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) {
    return (float)__builtin_bit_cast(_Float16, h);   // exact widening
}

__device__ __forceinline__ void adamw(float& p, float& m, float& v, float g, const SaeAdamStep hs, const SaeAdam a) {
    p = __fmul_rn(p, hs.decay);
    m = __fadd_rn(__fmul_rn(a.beta1, m), __fmul_rn(__fsub_rn(1.0f, a.beta1), g));
    v = __fadd_rn(__fmul_rn(a.beta2, v), __fmul_rn(__fmul_rn(__fsub_rn(1.0f, a.beta2), g), g));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), hs.bc2_sqrt), a.eps);
    p = __fsub_rn(p, __fmul_rn(hs.step_size, __fdiv_rn(m, denom)));
}

__global__ __launch_bounds__(256, 2) void rater_forward_kernel(const uint16_t* __restrict__ rows, int d, const uint32_t* __restrict__ tab,
                                                               size_t tab_stride, size_t first, size_t R, const float* __restrict__ up,
                                                               const float* __restrict__ bias, int vec, float* __restrict__ u_out,
                                                               float* __restrict__ h_out, const uint32_t* __restrict__ stop) {
    __shared__ float As[DM * D_LS];
    __shared__ float Bs[DN * D_LS];
    __shared__ unsigned long long src[DM];   // source row of each tile slot, ~0 past the end
    if (stop && *stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const size_t i0 = (size_t)blockIdx.x * DM, member = blockIdx.z;
    const int n0 = (int)blockIdx.y * DN;
    if (tid < DM) {
        const size_t gi = i0 + tid;
        src[tid] = gi < R ? (tab ? (unsigned long long)tab[member * tab_stride + gi] : (unsigned long long)(first + gi)) : ~0ull;
    }
    __syncthreads();
    // a thread fetches 16 consecutive k of ONE tile slot and of ONE hidden unit per k step
    const int fr = tid >> 1, fk = (tid & 1) * 16;
    const uint16_t* const ap = src[fr] != ~0ull ? rows + (size_t)src[fr] * d : nullptr;
    const float* const bp = n0 + fr < d ? up + (member * (size_t)d + (size_t)(n0 + fr)) * d : nullptr;
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
                for (int j = 0; j < 8; j++) ra[8 * q + j] = (float)v[j];
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
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
    // a 32-slot block of the tile without a slot is not multiplied (at B = 1 two of the 128 slots exist); nothing of it is stored
    const bool live0 = i0 + (size_t)(wm * 64) < R, live1 = i0 + (size_t)(wm * 64 + 32) < R;
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += DK) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            As[fr * D_LS + fk + j] = ra[j];
            Bs[fr * D_LS + fk + j] = rb[j];
        }
        __syncthreads();
        if (k0 + DK < d) fetch(k0 + DK);
        if (live0) {
#pragma unroll
            for (int t = 0; t < DK / 2; t++) {
                const float a0 = As[(wm * 64 + l31) * D_LS + 2 * t + lh];
                const float b0 = Bs[(wn * 64 + l31) * D_LS + 2 * t + lh];
                const float b1 = Bs[(wn * 64 + 32 + l31) * D_LS + 2 * t + lh];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                if (live1) {
                    const float a1 = As[(wm * 64 + 32 + l31) * D_LS + 2 * t + lh];
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // this lane's two hidden units of the member are n0 + 64 wn + l31 and that + 32; register r of MFMA tile mt is tile slot
    // 64 wm + 32 mt + (r & 3) + 8 (r >> 2) + 4 lh
    const int c0 = n0 + wn * 64 + l31, c1 = c0 + 32;
    const bool in0 = c0 < d, in1 = c1 < d;
    const float bias0 = in0 ? bias[member * (size_t)d + c0] : 0.0f, bias1 = in1 ? bias[member * (size_t)d + c1] : 0.0f;
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const size_t gi = i0 + (size_t)(wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh);
            if (gi >= R) continue;
            const size_t at = (member * R + gi) * (size_t)d;
            if (in0) {
                const float u0 = __fadd_rn(acc[mt][0][r], bias0);
                if (u_out) u_out[at + c0] = u0;
                h_out[at + c0] = rater_silu(u0);
            }
            if (in1) {
                const float u1 = __fadd_rn(acc[mt][1][r], bias1);
                if (u_out) u_out[at + c1] = u1;
                h_out[at + c1] = rater_silu(u1);
            }
        }
}

// One wave per (member, slot)
__global__ __launch_bounds__(256) void rater_scores_kernel(const float* __restrict__ h, const float* __restrict__ down, int E, int M, int C, size_t R,
                                                           float* __restrict__ s, size_t s_member, size_t s_row, const uint32_t* __restrict__ stop) {
    if (stop && *stop) return;
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (size_t)M * R) return;
    const size_t m = w / R, r = w - m * R, H = (size_t)M * E;
    const float* hp = h + w * (size_t)E;
    const float* dp = down + m * (size_t)E;
    float S[MAX_CH];
#pragma unroll
    for (int c = 0; c < MAX_CH; c++) S[c] = 0.0f;
    for (int j = lane; j < E; j += 64) {
        const float hv = hp[j];
#pragma unroll
        for (int c = 0; c < MAX_CH; c++)
            if (c < C) S[c] = fmaf(hv, dp[(size_t)c * H + j], S[c]);
    }
#pragma unroll
    for (int c = 0; c < MAX_CH; c++) {
        if (c < C) {
            float v = S[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_down(v, o));   // lane l < o reads lane l + o, which the round before left whole
            if (lane == 0) s[m * s_member + r * s_row + c] = v;
        }
    }
}

// One wave per (member, slot): an f16 with all exponent bits set is an infinity or a NaN
__global__ __launch_bounds__(256) void rater_check_rows_kernel(RaterStep s) {
    if (s.ctl->stop) return;
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (size_t)s.M * 2 * s.B) return;
    const uint16_t* x = s.rows + (size_t)s.tab[w] * s.E;
    bool bad = false;
    for (int k = lane; k < s.E; k += 64) bad |= (x[k] & 0x7C00u) == 0x7C00u;
    if (bad) s.ctl->n_invalid = 1u;
}

// One workgroup.  The head of every (member, pair, channel), the loss in the stated order (a tile of 256 terms at a time through LDS,
// summed by one thread) and the gate
__global__ __launch_bounds__(256) void rater_head_kernel(RaterStep s) {
    __shared__ double tile[256];
    const int tid = threadIdx.x;
    if (s.ctl->stop) return;
    const int n = s.M * s.B * s.C, bc = s.B * s.C;
    double total = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        double term = 0.0;
        if (i < n) {
            const int m = i / bc, rem = i - m * bc, b = rem / s.C, c = rem - b * s.C;
            const size_t at = ((size_t)m * 2 * s.B + 2 * b) * s.C + c;
            const float z = __fsub_rn(s.s[at], s.s[at + s.C]);
            const float p = rater_sig(z), y = s.targets[i];
            s.g[i] = __fmul_rn(__fsub_rn(p, y), s.inv_n);
            const double pd = (double)p, yd = (double)y;
            double lp = log(pd), lq = log(1.0 - pd);
            lp = lp < -100.0 ? -100.0 : lp;
            lq = lq < -100.0 ? -100.0 : lq;
            term = -(yd * lp + (1.0 - yd) * lq);
        }
        tile[tid] = term;
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(256, n - base);
            for (int j = 0; j < cnt; j++) total = __dadd_rn(total, tile[j]);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double L = total / (double)n;
    const bool bad = s.ctl->n_invalid != 0 || !(L - L == 0.0);   // NaN and the infinities fail the comparison
    s.ctl->n_invalid = 0;
    if (bad) {
        s.ctl->stop = 1;
        return;
    }
    *s.loss = L;
    s.ctl->steps_done += 1;
}

__device__ __forceinline__ float slot_ds(const RaterStep& s, int m, int r, int c) {
    const float g = s.g[((size_t)m * s.B + (r >> 1)) * s.C + c];
    return (r & 1) ? -g : g;
}

// A thread per (member, slot, unit)
__global__ __launch_bounds__(256) void rater_du_kernel(RaterStep s) {
    if (s.ctl->stop) return;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, R = 2 * (size_t)s.B, E = (size_t)s.E;
    if (idx >= (size_t)s.M * R * E) return;
    const size_t slot = idx / E, j = idx - slot * E, m = slot / R, r = slot - m * R, H = (size_t)s.M * E;
    float dh = 0.0f;
    for (int c = 0; c < s.C; c++) dh = fmaf(slot_ds(s, (int)m, (int)r, c), s.down[(size_t)c * H + m * E + j], dh);
    s.du[idx] = __fmul_rn(dh, rater_silu_grad(s.u[idx]));
}

// A thread per element of down; runs after rater_du_kernel, which reads down
__global__ __launch_bounds__(256) void rater_down_kernel(RaterStep s) {
    if (s.ctl->stop) return;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, R = 2 * (size_t)s.B, E = (size_t)s.E, H = (size_t)s.M * E;
    if (idx >= (size_t)s.C * H) return;
    const size_t c = idx / H, unit = idx - c * H, m = unit / E, j = unit - m * E;
    float g = 0.0f;
    for (size_t r = 0; r < R; r++) g = fmaf(slot_ds(s, (int)m, (int)r, (int)c), s.h[(m * R + r) * E + j], g);
    float p = s.down[idx], mm = s.m_down[idx], v = s.v_down[idx];
    adamw(p, mm, v, g, *s.hyper, s.adam);
    s.down[idx] = p;
    s.m_down[idx] = mm;
    s.v_down[idx] = v;
}

__global__ __launch_bounds__(256) void rater_bias_kernel(RaterStep s) {
    if (s.ctl->stop) return;
    const size_t unit = (size_t)blockIdx.x * 256 + threadIdx.x, R = 2 * (size_t)s.B, E = (size_t)s.E;
    if (unit >= (size_t)s.M * E) return;
    const size_t m = unit / E, j = unit - m * E;
    float g = 0.0f;
    for (size_t r = 0; r < R; r++) g = __fadd_rn(g, s.du[(m * R + r) * E + j]);
    float p = s.bias[unit], mm = s.m_bias[unit], v = s.v_bias[unit];
    adamw(p, mm, v, g, *s.hyper, s.adam);
    s.bias[unit] = p;
    s.m_bias[unit] = mm;
    s.v_bias[unit] = v;
}

// The dense pass.  A thread takes W = 4 consecutive k of one unit's row (16 bytes of each of the three arrays) where rows are 16-byte
// aligned, one float otherwise, and walks the array with the grid's stride.  The gradient of its W elements is the chain over the
// member's slots, whose du and x (a few MB per step) come from L2; the three streams are read and written once and do not displace
// them (non-temporal)
template <bool VEC>
__global__ __launch_bounds__(256) void rater_update_kernel(RaterStep s) {
    if (s.ctl->stop) return;
    constexpr int W = VEC ? 4 : 1;
    const SaeAdamStep hs = *s.hyper;
    const size_t E = (size_t)s.E, R = 2 * (size_t)s.B, cpr = E / W, total = (size_t)s.M * E * cpr;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < total; c += (size_t)gridDim.x * 256) {
        const size_t unit = c / cpr, k = (c - unit * cpr) * W, m = unit / E, j = unit - m * E;
        float g[W];
#pragma unroll
        for (int q = 0; q < W; q++) g[q] = 0.0f;
        const uint32_t* tab = s.tab + m * R;
        const float* du = s.du + m * R * E + j;
        for (size_t r = 0; r < R; r++) {
            const float dv = du[r * E];
            const uint16_t* x = s.rows + (size_t)tab[r] * E + k;
            if constexpr (VEC) {
                const uint2 xv = *reinterpret_cast<const uint2*>(x);
                g[0] = fmaf(dv, f16_bits_to_f32((uint16_t)xv.x), g[0]);
                g[1] = fmaf(dv, f16_bits_to_f32((uint16_t)(xv.x >> 16)), g[1]);
                g[2] = fmaf(dv, f16_bits_to_f32((uint16_t)xv.y), g[2]);
                g[3] = fmaf(dv, f16_bits_to_f32((uint16_t)(xv.y >> 16)), g[3]);
            } else {
                g[0] = fmaf(dv, f16_bits_to_f32(x[0]), g[0]);
            }
        }
        const size_t at = unit * E + k;
        if constexpr (VEC) {
            f32x4 pu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.up + at));
            f32x4 mu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.m_up + at));
            f32x4 vu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.v_up + at));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float p = pu[q], mm = mu[q], v = vu[q];
                adamw(p, mm, v, g[q], hs, s.adam);
                pu[q] = p; mu[q] = mm; vu[q] = v;
            }
            __builtin_nontemporal_store(pu, reinterpret_cast<f32x4*>(s.up + at));
            __builtin_nontemporal_store(mu, reinterpret_cast<f32x4*>(s.m_up + at));
            __builtin_nontemporal_store(vu, reinterpret_cast<f32x4*>(s.v_up + at));
        } else {
            float p = s.up[at], mm = s.m_up[at], v = s.v_up[at];
            adamw(p, mm, v, g[0], hs, s.adam);
            s.up[at] = p; s.m_up[at] = mm; s.v_up[at] = v;
        }
    }
}

// A thread per pair
__global__ __launch_bounds__(256) void rater_pair_variance_kernel(const float* __restrict__ table, int M, int C, const uint32_t* __restrict__ a_idx,
                                                                  const uint32_t* __restrict__ b_idx, size_t n_pairs, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const float* sa = table + (size_t)a_idx[i] * M * C;
    const float* sb = table + (size_t)b_idx[i] * M * C;
    float best = 0.0f;
    for (int c = 0; c < C; c++) {
        float sum = 0.0f;
        for (int m = 0; m < M; m++) sum = __fadd_rn(sum, rater_sig(__fsub_rn(sa[m * C + c], sb[m * C + c])));
        const float mean = __fdiv_rn(sum, (float)M);
        float acc = 0.0f;
        for (int m = 0; m < M; m++) {
            const float dlt = __fsub_rn(rater_sig(__fsub_rn(sa[m * C + c], sb[m * C + c])), mean);
            acc = __fadd_rn(acc, __fmul_rn(dlt, dlt));
        }
        const float var = __fdiv_rn(acc, (float)(M - 1));
        best = c == 0 ? var : (var > best ? var : best);
    }
    out[i] = best;
}

}  // namespace

void launch_rater_forward(const uint16_t* rows, int E, int M, const uint32_t* tab, size_t tab_stride, size_t first, size_t R, const float* up,
                          const float* bias, float* u_or_null, float* h, const uint32_t* stop_or_null, hipStream_t st) {
    if (R == 0) return;
    const int vec = E % 8 == 0 && (((uintptr_t)rows | (uintptr_t)up) & 15) == 0;   // every row and weight row starts 16-byte aligned
    const dim3 grid((unsigned)((R + DM - 1) / DM), (unsigned)((E + DN - 1) / DN), (unsigned)M);
    hipLaunchKernelGGL(rater_forward_kernel, grid, dim3(256), 0, st, rows, E, tab, tab_stride, first, R, up, bias, vec, u_or_null, h, stop_or_null);
}

void launch_rater_scores(const float* h, const float* down, int E, int M, int C, size_t R, float* s, size_t s_member, size_t s_row,
                         const uint32_t* stop_or_null, hipStream_t st) {
    if (R == 0) return;
    const size_t waves = (size_t)M * R;
    hipLaunchKernelGGL(rater_scores_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, h, down, E, M, C, R, s, s_member, s_row, stop_or_null);
}

void launch_rater_backward(const RaterStep& s, hipStream_t st) {
    const size_t R = 2 * (size_t)s.B, E = (size_t)s.E, H = (size_t)s.M * E;
    hipLaunchKernelGGL(rater_check_rows_kernel, dim3((unsigned)(((size_t)s.M * R + 3) / 4)), dim3(256), 0, st, s);
    hipLaunchKernelGGL(rater_head_kernel, dim3(1), dim3(256), 0, st, s);
    hipLaunchKernelGGL(rater_du_kernel, dim3((unsigned)((H * R + 255) / 256)), dim3(256), 0, st, s);
    hipLaunchKernelGGL(rater_down_kernel, dim3((unsigned)(((size_t)s.C * H + 255) / 256)), dim3(256), 0, st, s);
    hipLaunchKernelGGL(rater_bias_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, s);
}

void launch_rater_update(const RaterStep& s, hipStream_t st) {
    const uintptr_t all = (uintptr_t)s.up | (uintptr_t)s.m_up | (uintptr_t)s.v_up;
    const bool vec = s.E % 4 == 0 && (all & 15) == 0 && ((uintptr_t)s.rows & 7) == 0;
    const size_t E = (size_t)s.E, total = (size_t)s.M * E * (vec ? E / 4 : E);
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, (size_t)s.n_cu * 16));
    if (vec) hipLaunchKernelGGL(rater_update_kernel<true>, dim3(grid), dim3(256), 0, st, s);
    else hipLaunchKernelGGL(rater_update_kernel<false>, dim3(grid), dim3(256), 0, st, s);
}

void launch_rater_pair_variance(const float* table, int M, int C, const uint32_t* a_idx, const uint32_t* b_idx, size_t n_pairs, float* out,
                                hipStream_t st) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(rater_pair_variance_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, table, M, C, a_idx, b_idx, n_pairs, out);
}

}  // namespace mse
