// Sparse-autoencoder training over a resident index (sae/train.py:51-59 of the reference: mse_loss, backward, torch.optim.AdamW): the
// backward pass and the optimizer of one step.  The forward pass is sae.hip's kernels, called and not changed.
//
//   sae_train_gate_kernel      the step's loss, its pair count and the gate
//   sae_train_rank_kernel      the pair index: every kept (row, feature) pair at its rank in (feature, row) order
//   sae_train_map_kernel       feature -> member range, the touched flags, the feature counters
//   sae_train_grad_out_kernel  gR, the decoder bias's gradient and its AdamW update
//   sae_train_hidden_kernel    the hidden gradient of every pair, one wave each
//   sae_train_up_bias_kernel   the encoder bias's gradient and update
//   sae_train_update_kernel    ONE pass over the d_hidden rows of up and downT and their four moment arrays: a row's gradient is formed
//                              on the fly from its members; no [d_hidden][d_emb] gradient exists
//   sae_train_unmap_kernel     the member map back to empty
//
// THE RULE (tests/sae_train_ref.py restates it; bit for bit).  B rows of a step (entries of an id list: the same id may come twice),
// E = d_emb, H = d_hidden, K = top_k; f32 parameters up [H][E], up_bias [H] (optional), downT [H][E] (down transposed), down_bias [E];
// every parameter with moments m and v of its shape; one step count t.
//   forward     sae.hip's rule: counts, canonical features and activations a, the reconstruction r, the f64 squared error of every row
//   gate        a step with an invalid (NaN) row or a non-finite loss is refused: weights, moments, t and counters stay, later steps of
//               the call are not run
//   loss        L = (sum of sqerr_i, i ascending from +0, f64 adds) / (double)(B E)
//   gR          e = f32(r - x) as in the squared error; gR[i][d] = e * s, one f32 multiply, s = (float)(2.0 / (double)(B E))
//   pairs       the kept (i, f), grouped by feature, a feature's members in ascending i (the order is unique).  B K <= 65536
//   hidden      h(i, f) = sum over d of downT[f][d] gR[i][d] with the weights from BEFORE the update: 64 lanes, lane l the chain
//               S_l = fma(downT[f][d], gR[i][d], S_l) over d = l, l + 64, ... ascending from +0 (a lane without a d holds +0), then the
//               tree S_l = S_l + S_{l + o}, o = 32, 16, ..., 1, l < o; h = S_0.  The threshold carries no gradient; the mask is the
//               strict one, so a feature that ties at the threshold has no pair
//   gradients   each one chain from +0 over the feature's members in ascending i:
//               g_up[f][k] = fma(h, x[i][k], g); g_downT[f][d] = fma(a, gR[i][d], g); g_up_bias[f] = g + h;
//               g_down_bias[d] = g + gR[i][d] over ALL rows i ascending.  A feature without members has gradient +0
//   AdamW       elementwise f32, adam_kernel's form (pq_train.hip), torch's order (decoupled decay first):
//               p = p * decay; m = beta1 m + (1 - beta1) g; v = beta2 v + ((1 - beta2) g) g;
//               p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps)), every operation rounded once -- the square root and the quotients
//               correctly (sqrtf and __fdiv_rn; adam_kernel's __fsqrt_rn is the hardware's approximation and pins no bits);
//               decay = (float)(1 - lr wd), step_size = (float)(lr / (1 - beta1^t)), bc2_sqrt = (float)sqrt(1 - beta2^t) in double on
//               the host.  Every parameter moves at every step: a feature that did not fire moves by its momentum
//   counters    a completed step adds one per pair to its feature's u64 counter
// Nothing in it names the grid, the tile, ids versus host rows or how a call is cut into steps.
//
// SKIPPING.  With decay == 1 a feature row whose moments are all zero and which has no member does not move: m and v stay +0 and
// p - step_size * (0 / (0 / bc2_sqrt + eps)) = p - 0 = p (eps > 0; with eps = 0 the quotient is NaN and nothing is skipped).  `touched`
// marks the features that have had a member since their moments were zero; the others are not read.  The bytes are the same.
#include "sae_train.h"
#include "sae.h"

namespace mse {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u64 = unsigned long long;
constexpr int UPD_ROWS = 8;   // feature rows a workgroup of the dense pass takes at a time

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

__device__ __forceinline__ size_t source_row(const SaeTrainStep& s, uint32_t i) {
    return s.ids ? (size_t)s.ids[i] : s.first + i;
}

// One workgroup.  The loss in the stated order (a tile of 256 squared errors at a time through LDS, summed by one thread), the pair
// count, and the gate.  It also takes sae_merge_kernel's invalid-row count back to zero for the next step
__global__ __launch_bounds__(256) void sae_train_gate_kernel(SaeTrainStep s) {
    __shared__ double tile[256];
    __shared__ uint32_t np_s;
    const int tid = threadIdx.x;
    if (s.ctl->stop) return;
    if (tid == 0) np_s = 0;
    __syncthreads();
    uint32_t np = 0;
    for (int i = tid; i < s.B; i += 256) {
        const uint32_t c = s.counts[i];
        if (c != SAE_NONE) np += min(c, (uint32_t)s.K);
    }
    atomicAdd(&np_s, np);
    double total = 0.0;
    for (int base = 0; base < s.B; base += 256) {
        tile[tid] = base + tid < s.B ? s.sqerr[base + tid] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int m = min(256, s.B - base);
            for (int j = 0; j < m; j++) total = __dadd_rn(total, tile[j]);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double L = total / (double)((size_t)s.B * (size_t)s.E);
    const bool bad = s.ctl->n_invalid != 0 || !(L - L == 0.0);   // NaN and the infinities fail the comparison
    s.ctl->n_invalid = 0;
    if (bad) {
        s.ctl->stop = 1;
        return;
    }
    *s.loss = L;
    s.ctl->steps_done += 1;
    s.ctl->n_pairs = np_s;
}

// A thread per slot of the step's [B][K] feature table.  The key of a kept slot is feature << 32 | row: distinct, and ordered as the
// pair index is.  Its rank is the number of smaller keys, counted against every slot, a tile of 256 keys at a time through LDS
__global__ __launch_bounds__(256) void sae_train_rank_kernel(SaeTrainStep s) {
    __shared__ u64 keys[256];
    if (s.ctl->stop) return;
    const int tid = threadIdx.x;
    const uint32_t slots = (uint32_t)s.B * (uint32_t)s.K;
    auto key_of = [&](uint32_t q) -> u64 {
        if (q >= slots) return ~0ull;
        const uint32_t i = q / (uint32_t)s.K, j = q - i * (uint32_t)s.K, c = s.counts[i];
        if (c == SAE_NONE || j >= c) return ~0ull;
        return ((u64)s.feats[q] << 32) | i;
    };
    const uint32_t q = blockIdx.x * 256u + tid;
    const u64 mine = key_of(q);
    uint32_t rank = 0;
    for (uint32_t base = 0; base < slots; base += 256) {
        keys[tid] = key_of(base + tid);
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < 256; j++) rank += keys[j] < mine ? 1u : 0u;
        __syncthreads();
    }
    if (mine == ~0ull || rank >= slots) return;
    s.p_row[rank] = (uint32_t)mine;
    s.p_feat[rank] = (uint32_t)(mine >> 32);
    s.p_act[rank] = s.acts[q];
}

__global__ __launch_bounds__(256) void sae_train_map_kernel(SaeTrainStep s) {
    if (s.ctl->stop) return;
    const uint32_t n = s.ctl->n_pairs, p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t f = s.p_feat[p];
    if (f >= (uint32_t)s.H) return;
    if (p == 0 || s.p_feat[p - 1] != f) s.fmap[f].x = p;
    if (p + 1 == n || s.p_feat[p + 1] != f) s.fmap[f].y = p + 1;
    s.touched[f] = 1;
    atomicAdd(&s.counters[f], 1ull);
}

__global__ __launch_bounds__(256) void sae_train_unmap_kernel(SaeTrainStep s) {
    if (s.ctl->stop) return;
    const uint32_t n = s.ctl->n_pairs, p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t f = s.p_feat[p];
    if (f < (uint32_t)s.H) s.fmap[f] = make_uint2(0u, 0u);
}

// A thread per component d: gR[i][d] for every row and, along the way, the decoder bias's gradient; then its update
__global__ __launch_bounds__(256) void sae_train_grad_out_kernel(SaeTrainStep s, float gscale) {
    if (s.ctl->stop) return;
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= s.E) return;
    float g = 0.0f;
    for (int i = 0; i < s.B; i++) {
        const float x = f16_bits_to_f32(s.rows[source_row(s, (uint32_t)i) * s.E + d]);
        const float e = __fsub_rn(s.recon[(size_t)i * s.E + d], x);
        const float gr = __fmul_rn(e, gscale);
        s.gR[(size_t)i * s.E + d] = gr;
        g = __fadd_rn(g, gr);
    }
    float p = s.down_bias[d], m = s.m_db[d], v = s.v_db[d];
    adamw(p, m, v, g, *s.hyper, s.adam);
    s.down_bias[d] = p;
    s.m_db[d] = m;
    s.v_db[d] = v;
}

// One wave per pair
__global__ __launch_bounds__(256) void sae_train_hidden_kernel(SaeTrainStep s) {
    if (s.ctl->stop) return;
    const int lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= s.ctl->n_pairs) return;
    const uint32_t i = s.p_row[p], f = s.p_feat[p];
    const float* w = s.downT + (size_t)f * s.E;
    const float* g = s.gR + (size_t)i * s.E;
    float S = 0.0f;
    for (int d = lane; d < s.E; d += 64) S = fmaf(w[d], g[d], S);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) S = __fadd_rn(S, __shfl_down(S, o));   // lane l < o reads lane l + o, which the round before left whole
    if (lane == 0) s.p_h[p] = S;
}

__global__ __launch_bounds__(256) void sae_train_up_bias_kernel(SaeTrainStep s) {
    if (s.ctl->stop) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= s.H) return;
    const uint2 r = s.fmap[f];
    float g = 0.0f;
    for (uint32_t p = r.x; p < r.y; p++) g = __fadd_rn(g, s.p_h[p]);
    float q = s.up_bias[f], m = s.m_ub[f], v = s.v_ub[f];
    adamw(q, m, v, g, *s.hyper, s.adam);
    s.up_bias[f] = q;
    s.m_ub[f] = m;
    s.v_ub[f] = v;
}

// The dense pass.  A workgroup takes UPD_ROWS feature rows at a time and its threads walk their elements -- W = 4 floats (16 bytes of
// each of the six arrays) per thread where rows are 16-byte aligned, one float otherwise.  The gradient of the thread's W elements of
// up and of downT is the chain over the row's members, whose x, gR, h and a (a few hundred KB per step) come from L2; the six streams
// are read and written once and do not displace them (non-temporal)
template <bool VEC>
__global__ __launch_bounds__(256) void sae_train_update_kernel(SaeTrainStep s) {
    if (s.ctl->stop) return;
    constexpr int W = VEC ? 4 : 1;
    const SaeAdamStep hs = *s.hyper;
    const uint32_t E = (uint32_t)s.E, H = (uint32_t)s.H, cpr = E / W, span = UPD_ROWS * cpr;
    const uint32_t groups = (H + UPD_ROWS - 1) / UPD_ROWS;
    for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const uint32_t f0 = grp * UPD_ROWS;
        for (uint32_t c = threadIdx.x; c < span; c += 256) {
            const uint32_t fr = c / cpr, f = f0 + fr, k = (c - fr * cpr) * W;
            if (f >= H) break;
            const uint2 r = s.fmap[f];
            if (s.skip && r.x == r.y && !s.touched[f]) continue;
            float gu[W], gd[W];
#pragma unroll
            for (int j = 0; j < W; j++) gu[j] = gd[j] = 0.0f;
            for (uint32_t p = r.x; p < r.y; p++) {
                const uint32_t i = s.p_row[p];
                const float h = s.p_h[p], a = s.p_act[p];
                const uint16_t* x = s.rows + source_row(s, i) * E + k;
                const float* g = s.gR + (size_t)i * E + k;
                float xs[W], gs[W];
                if constexpr (VEC) {
                    const uint2 xv = *reinterpret_cast<const uint2*>(x);
                    xs[0] = f16_bits_to_f32((uint16_t)xv.x); xs[1] = f16_bits_to_f32((uint16_t)(xv.x >> 16));
                    xs[2] = f16_bits_to_f32((uint16_t)xv.y); xs[3] = f16_bits_to_f32((uint16_t)(xv.y >> 16));
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(g);
#pragma unroll
                    for (int j = 0; j < W; j++) gs[j] = gv[j];
                } else {
                    xs[0] = f16_bits_to_f32(x[0]);
                    gs[0] = g[0];
                }
#pragma unroll
                for (int j = 0; j < W; j++) {
                    gu[j] = fmaf(h, xs[j], gu[j]);
                    gd[j] = fmaf(a, gs[j], gd[j]);
                }
            }
            const size_t at = (size_t)f * E + k;
            if constexpr (VEC) {
                f32x4 pu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.up + at));
                f32x4 mu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.m_up + at));
                f32x4 vu = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.v_up + at));
                f32x4 pd = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.downT + at));
                f32x4 md = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.m_down + at));
                f32x4 vd = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s.v_down + at));
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float p = pu[j], m = mu[j], v = vu[j];
                    adamw(p, m, v, gu[j], hs, s.adam);
                    pu[j] = p; mu[j] = m; vu[j] = v;
                    p = pd[j]; m = md[j]; v = vd[j];
                    adamw(p, m, v, gd[j], hs, s.adam);
                    pd[j] = p; md[j] = m; vd[j] = v;
                }
                __builtin_nontemporal_store(pu, reinterpret_cast<f32x4*>(s.up + at));
                __builtin_nontemporal_store(mu, reinterpret_cast<f32x4*>(s.m_up + at));
                __builtin_nontemporal_store(vu, reinterpret_cast<f32x4*>(s.v_up + at));
                __builtin_nontemporal_store(pd, reinterpret_cast<f32x4*>(s.downT + at));
                __builtin_nontemporal_store(md, reinterpret_cast<f32x4*>(s.m_down + at));
                __builtin_nontemporal_store(vd, reinterpret_cast<f32x4*>(s.v_down + at));
            } else {
                float p = s.up[at], m = s.m_up[at], v = s.v_up[at];
                adamw(p, m, v, gu[0], hs, s.adam);
                s.up[at] = p; s.m_up[at] = m; s.v_up[at] = v;
                p = s.downT[at]; m = s.m_down[at]; v = s.v_down[at];
                adamw(p, m, v, gd[0], hs, s.adam);
                s.downT[at] = p; s.m_down[at] = m; s.v_down[at] = v;
            }
        }
    }
}

}  // namespace

void launch_sae_train_gate(const SaeTrainStep& s, hipStream_t st) {
    hipLaunchKernelGGL(sae_train_gate_kernel, dim3(1), dim3(256), 0, st, s);
}

void launch_sae_train_backward(const SaeTrainStep& s, hipStream_t st) {
    const unsigned slots = (unsigned)s.B * (unsigned)s.K, slot_blocks = (slots + 255) / 256;
    const float gscale = (float)(2.0 / (double)((size_t)s.B * (size_t)s.E));
    hipLaunchKernelGGL(sae_train_rank_kernel, dim3(slot_blocks), dim3(256), 0, st, s);
    hipLaunchKernelGGL(sae_train_map_kernel, dim3(slot_blocks), dim3(256), 0, st, s);
    hipLaunchKernelGGL(sae_train_grad_out_kernel, dim3((unsigned)(s.E + 255) / 256), dim3(256), 0, st, s, gscale);
    hipLaunchKernelGGL(sae_train_hidden_kernel, dim3((slots + 3) / 4), dim3(256), 0, st, s);
    if (s.up_bias) hipLaunchKernelGGL(sae_train_up_bias_kernel, dim3((unsigned)(s.H + 255) / 256), dim3(256), 0, st, s);
}

void launch_sae_train_update(const SaeTrainStep& s, hipStream_t st) {
    const uintptr_t all = (uintptr_t)s.up | (uintptr_t)s.m_up | (uintptr_t)s.v_up | (uintptr_t)s.downT | (uintptr_t)s.m_down | (uintptr_t)s.v_down |
                          (uintptr_t)s.gR;
    const bool vec = s.E % 4 == 0 && (all & 15) == 0 && ((uintptr_t)s.rows & 7) == 0;
    const unsigned groups = ((unsigned)s.H + UPD_ROWS - 1) / UPD_ROWS;
    const unsigned grid = std::max(1u, std::min(groups, (unsigned)s.n_cu * 8u));
    if (vec) hipLaunchKernelGGL(sae_train_update_kernel<true>, dim3(grid), dim3(256), 0, st, s);
    else hipLaunchKernelGGL(sae_train_update_kernel<false>, dim3(grid), dim3(256), 0, st, s);
    const unsigned slots = (unsigned)s.B * (unsigned)s.K;
    hipLaunchKernelGGL(sae_train_unmap_kernel, dim3((slots + 255) / 256), dim3(256), 0, st, s);
}

}  // namespace mse
