// Sparse-autoencoder features of a resident index (sae/model.py:31-43 of the reference, over the base's f16 rows):
//
//   sae_encode_kernel        relu(up . x (+ up_bias)) on the f32 matrix cores, streamed over d_hidden: per row the best top_k + 1 activations
//                            of one part of the hidden units; the [rows][d_hidden] activations are never written
//   sae_merge_kernel         the best top_k + 1 of the parts' lists, the strict `>` rule of model.py:34-41, canonical order, counters
//   sae_reconstruct_kernel   down . a + down_bias over the kept features from a [d_hidden][d_emb] copy of down, and the row's squared error
//                            (sae/train.py:55-56)
//   sae_feature_bits_kernel  the bitmap of the rows that keep one feature, for mse_filter_from_bits_dev
//   sae_transpose_kernel     that copy of down, made once at load
//
// THE RULE (tests/sae_ref.py restates it; bit for bit):
//   pre-activation  z_j = fma(up[j][K-1], x[K-1], ... fma(up[j][0], x[0], +0)): v_mfma_f32_32x32x2_f32 is a k-ordered f32 fma chain and one
//                   wave feeds one output its k pairs in ascending order (score_mlp_kernel of describe.hip: the same tile, loads and k
//                   pipeline, restated here so that describe.hip compiles as it did).  With a bias: z_j = z_j + up_bias[j], one f32 add
//   relu            a_j = z_j where z_j > 0, else +0 (so -0.0 is never positive)
//   threshold       t = the (top_k + 1)-th largest a_j (torch.kthvalue(a, d_hidden - top_k)); kept = { j : a_j > t }
//   order           activation descending, then feature ascending; unused slots hold feature 0xFFFFFFFF and activation +0
//   NaN             a row with a NaN z_j is invalid: count 0xFFFFFFFF, no features, nothing counted.  +inf is an ordinary value
//   reconstruction  r_d = fma(a, downT[f][d], r_d) over the kept features in that order, from down_bias[d] (or +0)
//   squared error   e_d = f32(r_d - x_d); S_t = sum of f64(e_d)^2 over d = t, t + 256, t + 512, ... ascending from +0, t < 256; then the
//                   tree S_t = S_t + S_{t + o} for o = 128, 64, ..., 1, t < o; the row's error is S_0.  An invalid row gives NaN
// None of this names the row's place in its tile, the call's size, ids versus range, the grid or how d_hidden is split.
//
// SELECTION.  A positive f32 orders as its bits, so a candidate is the key u64 = bits(z) << 32 | ~j: keys are distinct, and key order is
// (activation descending, feature ascending).  Each (row, part) has a running threshold key, 0 at first: an activation becomes a candidate
// only if its key exceeds it.  Candidates are appended to the (row, part) list with a workgroup-local (LDS) atomic on the list's length.
// A hidden tile adds at most 128 entries to a row; a list holds top_k + 1 + 128 + 256 entries, and after a tile a list that the next tile
// could overflow (more than top_k + 1 + 256 entries) is cut to its best top_k + 1, the least of which becomes the threshold: a key at or
// below the running (top_k + 1)-th largest cannot be among the final top_k + 1.  The 256 entries of slack are what keeps the cuts rare:
// without them every candidate that arrives after a cut would force the next one.  A cut costs 64 rounds of compare-and-count over the
// lanes' registers (the k1-th largest key, bit by bit), no sort.  When its part is done a list is cut once more and sorted.  The top
// top_k + 1 of a union is the top top_k + 1 of the parts' tops, so the merge's answer does not depend on the split.
//
// WHERE THE LISTS LIVE.  128 rows x (top_k + 1 + 384) keys x 8 B is 513 KB at top_k = 128: no LDS holds it.  The lists are a slab of
// global memory per workgroup -- which is also the part's result, read by the merge -- and only their lengths, the thresholds and the NaN
// flags (2.5 KB) are in LDS.  After the first few tiles about top_k / d_hidden of the activations pass the threshold, so the slab sees a
// handful of 8-byte stores per tile and is re-read only by the rare cut: it stays in L2.  The final sort stages a list in the A tile's
// LDS (idle by then), ranks every entry against all others, and stores each at its rank.
#include "sae.h"

namespace mse {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
using u64 = unsigned long long;
constexpr int DM = SAE_ROW_TILE, DN = SAE_HID_TILE, DK = 32;
constexpr int D_LS = DK + 1;          // [row or unit][k], odd stride: the 32 rows of a half-wave land in 32 banks
constexpr int K1_MAX = SAE_MAX_TOP_K + 1;
constexpr int SLACK = SAE_LIST_SLACK;
constexpr int CAP_MAX = K1_MAX + DN + SLACK;          // 641
constexpr int SLOTS = (CAP_MAX + 63) / 64;            // list entries a lane holds during a cut
constexpr int SORT_SLOTS = (K1_MAX + 63) / 64;        // ... and during the final sort
constexpr int STAGE = SORT_SLOTS * 64;                // u64 per wave of the sort's staging area

__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) {
    return (float)__builtin_bit_cast(_Float16, h);   // exact widening
}

// One whole wave: the n (k1 < n <= cap) keys of `list` cut to the best k1, in place and in no particular order; returns the k1-th
// largest.  It is found bit by bit from the top -- the largest T with at least k1 keys >= T; keys are distinct, so exactly k1 are -- with
// the counts taken from the compare masks, so no lane waits for another
__device__ __forceinline__ u64 cut_list(u64* __restrict__ list, int n, int k1, int lane) {
    u64 mine[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        const int i = lane + 64 * j;
        mine[j] = (64 * j < n && i < n) ? list[i] : 0ull;   // an absent entry is below every candidate T
    }
    u64 T = 0;
    for (int bit = 63; bit >= 0; bit--) {
        const u64 cand = T | (1ull << bit);
        int c = 0;
#pragma unroll
        for (int j = 0; j < SLOTS; j++)
            if (64 * j < n) c += __builtin_popcountll(__ballot(mine[j] >= cand));
        if (c >= k1) T = cand;
    }
    int base = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        if (64 * j < n) {
            const bool keep = mine[j] >= T;
            const u64 mask = __ballot(keep);
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (keep && pos < k1) list[pos] = mine[j];
            base += __builtin_popcountll(mask);
        }
    }
    return T;
}

// One whole wave: the n (<= k1) keys of `list` sorted descending, in place.  Every key is ranked against all of them.  stage: LDS of
// this wave
__device__ __forceinline__ void sort_list(u64* __restrict__ list, int n, u64* stage, int lane) {
    u64 mine[SORT_SLOTS];
    int rank[SORT_SLOTS];
#pragma unroll
    for (int j = 0; j < SORT_SLOTS; j++) {
        const int i = lane + 64 * j;
        mine[j] = i < n ? list[i] : 0ull;
        rank[j] = 0;
        if (i < n) stage[i] = mine[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
    for (int m = 0; m < n; m++) {
        const u64 v = stage[m];
#pragma unroll
        for (int j = 0; j < SORT_SLOTS; j++) rank[j] += v > mine[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < SORT_SLOTS; j++)
        if (lane + 64 * j < n && rank[j] < n) list[rank[j]] = mine[j];
}

__global__ __launch_bounds__(256, 2) void sae_encode_kernel(const uint16_t* __restrict__ rows, int d, const uint32_t* __restrict__ ids, size_t first,
                                                            size_t n, const float* __restrict__ up, const float* __restrict__ up_bias,
                                                            int d_hidden, int k1, int tiles_per_part, int vec, u64* __restrict__ lists,
                                                            uint32_t* __restrict__ pcount, uint32_t* __restrict__ pflag) {
    __shared__ __attribute__((aligned(16))) float As[DM * D_LS];
    __shared__ float Bs[DN * D_LS];
    __shared__ u64 src[DM];    // base row of each tile row, ~0 past the end
    __shared__ u64 thr[DM];    // running threshold key of each tile row; ~0 past the end: nothing is a candidate
    __shared__ uint32_t cnt[DM];
    __shared__ uint32_t bad[DM];
    static_assert(4 * STAGE * 2 <= DM * D_LS, "the staging area of the four waves lies in the A tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int part = blockIdx.y, parts = gridDim.y;
    const int cap = k1 + DN + SLACK;
    const size_t i0 = (size_t)blockIdx.x * DM;
    if (tid < DM) {
        const size_t gi = i0 + tid;
        src[tid] = gi < n ? (ids ? (u64)ids[gi] : (u64)(first + gi)) : ~0ull;
        thr[tid] = gi < n ? 0ull : ~0ull;
        cnt[tid] = 0;
        bad[tid] = 0;
    }
    __syncthreads();
    u64* const slab = lists + (i0 * parts + part) * (size_t)cap;            // row r's list: slab + r * parts * cap
    const size_t row_stride = (size_t)parts * cap;
    u64* const stage = reinterpret_cast<u64*>(As) + wave * STAGE;
    // a thread fetches 16 consecutive k of ONE tile row and of ONE hidden unit per k step (score_mlp_kernel's loads)
    const int fr = tid >> 1, fk = (tid & 1) * 16;
    const uint16_t* const ap = src[fr] != ~0ull ? rows + (size_t)src[fr] * d : nullptr;
    const float* bp = nullptr;
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
                for (int j = 0; j < 8; j++) ra[8 * q + j] = (float)v[j];   // exact widening
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
    const int n_tiles = (d_hidden + DN - 1) / DN;
    const int t_begin = part * tiles_per_part;
    const int t_end = min(t_begin + tiles_per_part, n_tiles);
    for (int t = t_begin; t < t_end; t++) {
        const int n0 = t * DN;
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
            for (int s = 0; s < DK / 2; s++) {
                const float a0 = As[(wm * 64 + l31) * D_LS + 2 * s + lh];
                const float a1 = As[(wm * 64 + 32 + l31) * D_LS + 2 * s + lh];
                const float b0 = Bs[(wn * 64 + l31) * D_LS + 2 * s + lh];
                const float b1 = Bs[(wn * 64 + 32 + l31) * D_LS + 2 * s + lh];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            __syncthreads();
        }
        // epilogue in registers: this lane's two hidden units are n0 + 64 wn + l31 and that + 32; slot (mt, r) is tile row
        // 64 wm + 32 mt + (r & 3) + 8 (r >> 2) + 4 lh.  A unit past d_hidden is never a candidate and flags nothing
        const int c0 = n0 + wn * 64 + l31, c1 = c0 + 32;
        const bool in0 = c0 < d_hidden, in1 = c1 < d_hidden;
        const float bias0 = (up_bias && in0) ? up_bias[c0] : 0.0f, bias1 = (up_bias && in1) ? up_bias[c1] : 0.0f;
        const u64 low0 = (u64)(uint32_t)~(uint32_t)c0, low1 = (u64)(uint32_t)~(uint32_t)c1;
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const u64 th = thr[row];
                float z0 = acc[mt][0][r], z1 = acc[mt][1][r];
                if (up_bias) { z0 = __fadd_rn(z0, bias0); z1 = __fadd_rn(z1, bias1); }
                if ((in0 && z0 != z0) || (in1 && z1 != z1)) bad[row] = 1;
                if (in0 && z0 > 0.0f) {
                    const u64 key = ((u64)__builtin_bit_cast(uint32_t, z0) << 32) | low0;
                    if (key > th) {
                        const uint32_t pos = atomicAdd(&cnt[row], 1u);
                        if (pos < (uint32_t)cap) slab[row * row_stride + pos] = key;
                    }
                }
                if (in1 && z1 > 0.0f) {
                    const u64 key = ((u64)__builtin_bit_cast(uint32_t, z1) << 32) | low1;
                    if (key > th) {
                        const uint32_t pos = atomicAdd(&cnt[row], 1u);
                        if (pos < (uint32_t)cap) slab[row * row_stride + pos] = key;
                    }
                }
            }
        __syncthreads();
        // a list that the next tile could overflow is cut to its best k1, which raises the row's threshold; a wave takes every fourth row
        for (int row = wave; row < DM; row += 4) {
            const int c = __builtin_amdgcn_readfirstlane(min((int)cnt[row], cap));
            if (c + DN > cap) {
                const u64 t = cut_list(slab + row * row_stride, c, k1, lane);
                if (lane == 0) {
                    thr[row] = t;
                    cnt[row] = k1;
                }
            }
        }
        __syncthreads();   // the thresholds and lengths before the next epilogue
    }
    // the part's result: every list cut to its best k1 and sorted, its length and the row's flag
    for (int row = wave; row < DM; row += 4) {
        int c = __builtin_amdgcn_readfirstlane(min((int)cnt[row], cap));
        if (c > k1) {
            (void)cut_list(slab + row * row_stride, c, k1, lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the cut's stores before the sort's loads of other lanes' entries
            c = k1;
        }
        if (c > 1) sort_list(slab + row * row_stride, c, stage, lane);
        if (lane == 0 && i0 + row < n) {
            pcount[(i0 + row) * parts + part] = (uint32_t)c;
            pflag[(i0 + row) * parts + part] = bad[row];
        }
    }
}

// ---- merge -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// entries >= key of a descending list of c keys
__device__ __forceinline__ int count_ge(const u64* __restrict__ list, int c, u64 key) {
    int lo = 0, hi = c;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] >= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per row.  The k1-th largest key T of the union of the parts' sorted lists is found bit by bit from the top (the largest
// T with at least k1 keys >= T; keys are distinct, so exactly k1 are), the keys >= T are gathered and ranked, and the strict rule cuts them
__global__ __launch_bounds__(256) void sae_merge_kernel(const u64* __restrict__ lists, const uint32_t* __restrict__ pcount,
                                                        const uint32_t* __restrict__ pflag, int parts, int cap, int k1, size_t n,
                                                        uint32_t* __restrict__ counts, uint32_t* __restrict__ feats, float* __restrict__ acts,
                                                        u64* __restrict__ counters, uint32_t* __restrict__ n_invalid) {
    __shared__ u64 sel[K1_MAX];
    __shared__ u64 sorted[K1_MAX];
    __shared__ uint32_t red[4];
    __shared__ uint32_t scan[256];
    const int tid = threadIdx.x, top_k = k1 - 1;
    const size_t row = blockIdx.x;
    if (row >= n) return;
    const u64* const rl = lists + row * parts * (size_t)cap;
    const uint32_t* const rc = pcount + row * parts;
    uint32_t my_total = 0, my_bad = 0;
    for (int p = tid; p < parts; p += 256) {
        my_total += min(rc[p], (uint32_t)k1);
        my_bad += pflag[row * parts + p] ? 1u : 0u;
    }
    const uint32_t total = block_sum(my_total, red, tid);
    const uint32_t n_bad = block_sum(my_bad, red, tid);
    if (n_bad) {
        for (int i = tid; i < top_k; i += 256) {
            feats[row * top_k + i] = SAE_NONE;
            acts[row * top_k + i] = 0.0f;
        }
        if (tid == 0) {
            counts[row] = SAE_NONE;
            atomicAdd(n_invalid, 1u);
        }
        return;
    }
    u64 T = 0;
    if (total > (uint32_t)k1) {
        for (int bit = 63; bit >= 0; bit--) {
            const u64 cand = T | (1ull << bit);
            uint32_t c = 0;
            for (int p = tid; p < parts; p += 256) c += (uint32_t)count_ge(rl + (size_t)p * cap, (int)min(rc[p], (uint32_t)k1), cand);
            if (block_sum(c, red, tid) >= (uint32_t)k1) T = cand;
        }
    }
    uint32_t mine = 0;
    for (int p = tid; p < parts; p += 256) mine += (uint32_t)count_ge(rl + (size_t)p * cap, (int)min(rc[p], (uint32_t)k1), T);
    scan[tid] = mine;
    __syncthreads();
    uint32_t off = 0;
    for (int j = 0; j < tid; j++) off += scan[j];
    for (int p = tid; p < parts; p += 256) {
        const u64* l = rl + (size_t)p * cap;
        const int c = count_ge(l, (int)min(rc[p], (uint32_t)k1), T);
        for (int j = 0; j < c; j++, off++)
            if (off < (uint32_t)K1_MAX) sel[off] = l[j];
    }
    const int n_sel = (int)min(min(total, (uint32_t)k1), (uint32_t)K1_MAX);
    __syncthreads();
    for (int i = tid; i < n_sel; i += 256) {
        const u64 v = sel[i];
        int rank = 0;
        for (int m = 0; m < n_sel; m++) rank += sel[m] > v ? 1 : 0;
        sorted[rank] = v;
    }
    __syncthreads();
    // t = the k1-th largest activation, or 0 when fewer than k1 are positive; kept = the entries above it, a prefix of the sorted keys
    const uint32_t t_bits = n_sel == k1 ? (uint32_t)(sorted[k1 - 1] >> 32) : 0u;
    uint32_t kept_here = 0;
    for (int i = tid; i < top_k; i += 256) {
        const bool kept = i < n_sel && (uint32_t)(sorted[i] >> 32) > t_bits;
        const uint32_t f = kept ? ~(uint32_t)sorted[i] : SAE_NONE;
        feats[row * top_k + i] = f;
        acts[row * top_k + i] = kept ? __builtin_bit_cast(float, (uint32_t)(sorted[i] >> 32)) : 0.0f;
        if (kept) {
            kept_here++;
            if (counters) atomicAdd(&counters[f], 1ull);
        }
    }
    const uint32_t kept_all = block_sum(kept_here, red, tid);
    if (tid == 0) counts[row] = kept_all;
}

// ---- reconstruction ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sae_reconstruct_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ feats,
                                                              const float* __restrict__ acts, int top_k, const float* __restrict__ downT,
                                                              const float* __restrict__ down_bias, int d, const uint16_t* __restrict__ rows,
                                                              const uint32_t* __restrict__ ids, size_t first, size_t n, float* __restrict__ recon,
                                                              double* __restrict__ sqerr) {
    __shared__ uint32_t sf[SAE_MAX_TOP_K];
    __shared__ float sa[SAE_MAX_TOP_K];
    __shared__ double part[256];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    if (row >= n) return;
    const uint32_t c_raw = counts[row];
    const bool invalid = c_raw == SAE_NONE;
    const int c = invalid ? 0 : (int)min(c_raw, (uint32_t)top_k);
    if (tid < c) {
        sf[tid] = feats[row * top_k + tid];
        sa[tid] = acts[row * top_k + tid];
    }
    __syncthreads();
    const uint16_t* x = rows + (ids ? (size_t)ids[row] : first + row) * d;
    const float nan32 = __builtin_bit_cast(float, 0x7FC00000u);
    double s = 0.0;
    for (int e = tid; e < d; e += 256) {
        float r = down_bias ? down_bias[e] : 0.0f;
        for (int i = 0; i < c; i++) r = fmaf(sa[i], downT[(size_t)sf[i] * d + e], r);
        if (recon) recon[row * d + e] = invalid ? nan32 : r;
        const double err = (double)__fsub_rn(r, f16_bits_to_f32(x[e]));
        s = s + err * err;
    }
    part[tid] = s;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) part[tid] = part[tid] + part[tid + o];
    }
    if (tid == 0 && sqerr) sqerr[row] = invalid ? __builtin_bit_cast(double, 0x7FF8000000000000ull) : part[0];
}

__global__ __launch_bounds__(256) void sae_feature_bits_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ feats,
                                                               const float* __restrict__ acts, int top_k, size_t n, const uint32_t* __restrict__ ids,
                                                               size_t first, uint32_t feature, float min_activation, uint32_t* __restrict__ words) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = counts[i];
    if (c == SAE_NONE) return;
    bool hit = false;
    for (uint32_t j = 0; j < c && j < (uint32_t)top_k; j++)
        hit = hit || (feats[i * top_k + j] == feature && acts[i * top_k + j] >= min_activation);
    if (!hit) return;
    const size_t row = ids ? (size_t)ids[i] : first + i;
    atomicOr(&words[row >> 5], 1u << (row & 31));
}

__global__ __launch_bounds__(256) void sae_transpose_kernel(const float* __restrict__ down, size_t d_emb, size_t d_hidden, float* __restrict__ downT) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const size_t h0 = (size_t)blockIdx.x * 32, e0 = (size_t)blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8)
        if (e0 + j < d_emb && h0 + tx < d_hidden) tile[j][tx] = down[(e0 + j) * d_hidden + h0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (h0 + j < d_hidden && e0 + tx < d_emb) downT[(h0 + j) * d_emb + e0 + tx] = tile[tx][j];
}

}  // namespace

void launch_sae_transpose(const float* down, size_t d_emb, size_t d_hidden, float* downT, hipStream_t st) {
    hipLaunchKernelGGL(sae_transpose_kernel, dim3((unsigned)((d_hidden + 31) / 32), (unsigned)((d_emb + 31) / 32)), dim3(256), 0, st, down, d_emb,
                       d_hidden, downT);
}

void launch_sae_encode(const uint16_t* rows, int d, const uint32_t* ids, size_t first, size_t n, const float* up, const float* up_bias,
                       int d_hidden, int top_k, int parts, int tiles_per_part, unsigned long long* lists, uint32_t* pcount, uint32_t* pflag,
                       hipStream_t st) {
    const int vec = d % 8 == 0 && (((uintptr_t)rows | (uintptr_t)up) & 15) == 0;   // every row and weight row starts 16-byte aligned
    hipLaunchKernelGGL(sae_encode_kernel, dim3((unsigned)((n + DM - 1) / DM), (unsigned)parts), dim3(256), 0, st, rows, d, ids, first, n, up, up_bias,
                       d_hidden, top_k + 1, tiles_per_part, vec, lists, pcount, pflag);
}

void launch_sae_merge(const unsigned long long* lists, const uint32_t* pcount, const uint32_t* pflag, int parts, int top_k, size_t n,
                      uint32_t* counts, uint32_t* feats, float* acts, unsigned long long* counters, uint32_t* n_invalid, hipStream_t st) {
    hipLaunchKernelGGL(sae_merge_kernel, dim3((unsigned)n), dim3(256), 0, st, lists, pcount, pflag, parts, (int)sae_list_cap(top_k), top_k + 1, n,
                       counts, feats, acts, counters, n_invalid);
}

void launch_sae_reconstruct(const uint32_t* counts, const uint32_t* feats, const float* acts, int top_k, const float* downT, const float* down_bias,
                            int d, const uint16_t* rows, const uint32_t* ids, size_t first, size_t n, float* recon, double* sqerr, hipStream_t st) {
    hipLaunchKernelGGL(sae_reconstruct_kernel, dim3((unsigned)n), dim3(256), 0, st, counts, feats, acts, top_k, downT, down_bias, d, rows, ids, first,
                       n, recon, sqerr);
}

void launch_sae_feature_bits(const uint32_t* counts, const uint32_t* feats, const float* acts, int top_k, size_t n, const uint32_t* ids, size_t first,
                             uint32_t feature, float min_activation, uint32_t* words, hipStream_t st) {
    hipLaunchKernelGGL(sae_feature_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, counts, feats, acts, top_k, n, ids, first, feature,
                       min_activation, words);
}

}  // namespace mse
