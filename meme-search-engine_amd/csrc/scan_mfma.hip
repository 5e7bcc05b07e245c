// Batched brute-force scan on the matrix cores: candidate stage of the batched top-k.
//
// Reference work being replaced: the N x fast_dot loop of the brute-force evaluator
// (src/query_disk_index.rs:263-269) run for a whole batch of queries at once.  The matrix core sums
// the 1152 products in its own order, so these scores are NOT the reference's bit pattern; they only
// nominate candidate row groups.  Every candidate row is then re-scored in the reference order
// (scan_exact.hip) and a certificate (topk.hip::finalize_kernel) proves that no row outside the
// candidate groups can belong to the exact top-k; otherwise the caller widens the candidate set.
//
// Kernel: C[row, query] = sum_k X[row,k] * Q[query,k] with v_mfma_f32_16x16x32_f16, 8 waves per workgroup,
// one workgroup per CU (128 / 160 KiB of LDS), persistent grid-stride over 256-row tiles.  BN = queries per
// pass over the rows: 128, or 256 (round 2: the same HBM stream serves twice the queries; the matrix cores go
// from ~35 % to ~70 % busy, which is what the HBM-bound 128-query pass left idle).
//   - a wave owns 32 base rows (two 16-row MFMA tiles, A operand) x BN queries (BN/16 16-query column
//     tiles, B operand; each B fragment read from LDS feeds two MFMAs; 64 or 128 accumulator registers).
//   - base rows are streamed HBM -> LDS by the DMA path (global_load_lds, no VGPR staging).  Each wave DMAs
//     exactly the 32 rows x 128 B it will consume into its OWN ring of S stages (4 KiB each), so the
//     streamed operand needs no barrier: an LDS-DMA is ordered for a ds_read only by the issuing wave's
//     vmcnt, and that wait is counted by hand (the loads of a K block are always issued in the same order).
//     One DMA instruction moves 8 rows x 128 B, i.e. whole cache lines.  The LDS image of a DMA is
//     lane-linear, so the bank-conflict swizzle is applied to the SOURCE address: LDS slot (row, s) holds
//     global 16-byte piece s ^ f(row), f(row) = (row >> 1) & 7, and the A-fragment ds_read_b128 applies the
//     same involution (measured SQ_LDS_BANK_CONFLICT = 0).
//   - queries are re-tiled once per search into K-block-major, identically swizzled BN x 128 B tiles
//     (pack_queries_kernel); a tile is DMA'd linearly into a double buffer (BN/64 instructions per wave), one
//     barrier per 64-element K block.  The tile is shared by 256 rows, so L2->LDS query traffic is BN/256 of the
//     HBM traffic (it competes with the HBM stream for the CU's outstanding-miss slots).
//   - epilogue per 32-row group: max over the rows of each query column -> group_max[group][q]
//     (the level-0 array of the selection tournament).  4 bytes written per 32*2304 bytes read.  (The 320-query kernel's search
//     passes write one maximum per 64 rows, the rows of one wave: scan_mfma2d_kernel GR = 64.)
// Roofline: HBM.  Algorithmic bytes = 2*d per base row per pass of <= 128 queries; PMC FETCH_SIZE (x2 on
// gfx950, KiB) = 1.007 x that.
//
// Measured on MI355X at 1e7 x 1152 (profiles/): earlier variants of this kernel, kept here as a record of
// what did not work --  32x32x16 MFMA with lane = row (32 B per row per load instruction): 3.9-4.2 TB/s at
// every prefetch depth and occupancy; 16x16x32 with register-staged rows (64 B per row per instruction):
// 4.4-4.7 TB/s at 4 waves, 5.0-5.2 TB/s at 8 waves per workgroup; non-temporal loads on partial lines: -25 %;
// this DMA variant: 5.3-5.6 TB/s.  Ordinary (compiler-scheduled) loads are sunk next to their first use by
// hipcc, which leaves them no flight time; hence hand-issued DMA + counted waits.
//
// Round 2, the 256-query pass (1e7 x 1152, random rows, scan kernel alone; scripts/scan_ablate.py, MSE_SCAN_ABL):
//   128 queries 3.95-4.1 ms (HBM-bound, 5.6-5.8 TB/s) | 256 queries 5.65-5.75 ms = 4.0 TB/s, 1.04 PFLOP/s: +40 % queries/s.
//   Ablations of the 256-query kernel: MFMAs only 3.6 ms | X DMA only 3.9 | query-tile DMA only 0.83 | everything but the
//   MFMAs 4.1 | everything but the X DMA 4.5.  The parts do not hide behind each other the way the instruction counts
//   suggest, and re-timing them does not help: DMA pieces in one burst 5.90, one piece between MFMA groups (kept) 5.72,
//   bursts of the two waves of a SIMD half an iteration apart 6.30, a two-group ping-pong kernel (one wave per SIMD on the
//   matrix core while the other issues pieces, two barriers per K block) 6.06, nt loads for the rows: no change.  In-kernel
//   s_memtime stamps put the clock at 1.64 GHz under this load (2176 of 3400 cycles per K block are matrix-core cycles),
//   and the same kernel on all-zero rows -- same traffic, no operand toggling -- runs in 4.7 ms (MFMAs only: 3.0 ms):
//   the pass is bound by the chip's power budget (DVFS), not by a schedule.  LDS-DMA issue is not the limit either
//   (scripts/microbench/dma_rate.hip: 137 GB/s per CU from L2 with >= 4 waves, 7.5 ns per 1 KiB piece).  What would lower
//   the energy per row: wave tiles of 64 rows x 128 queries (a third fewer B-fragment LDS reads), not tried.
//   PMC counters (profiles/r02_pmc_scan_1e7.txt): 1.53 GHz and 62 % MFMA-busy at 256 queries, 1.84 GHz and 38 % at 128; both
//   passes pull ~19 B per cycle per CU through the vector L1 (rows + query tiles), which suggested that path as the bound --
//   but a 128-query kernel with 64 rows per wave (512-row tiles: a query tile fetched once per 512 rows, 17 % fewer L1 bytes
//   per row, 2-stage ring) ran 4.33 vs 4.20 ms at 1e7 rows and 42.0 vs 41.0 ms at 1e8: not that either.
//   Also without effect: v_mfma_f32_32x32x16_f16 over the same LDS images (half the MFMA instructions, one fragment read per
//   MFMA of twice the size; conflict-free with the same swizzle): 5.97 vs 5.80 ms; a 2-stage row ring instead of 3 (MSE_SCAN_S=2):
//   5.96 vs 5.95 ms at 256 queries, 4.25 vs 4.17 at 128 -- the pass is not limited by rows in flight; fragment reads issued by hand (asm ds_read_b128 + counted lgkmcnt waits instead of the
//   `s_waitcnt lgkmcnt(0)` hipcc puts in front of every MFMA group): 5.95 vs 6.06 ms on the same box, within noise.
//   Per K block (32 KiB of rows + 32 KiB of query tile through the CU's load path) the pass takes 2.1 us where the rows alone
//   take 1.4 us and the MFMAs alone 1.3 us; at 128 queries (48 KiB per K block) it takes 1.45 us.
#include "common.h"
#include "kernels.h"
#include <cstdlib>
#include <algorithm>
#include <type_traits>

namespace mse {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int KB = 64;            // contraction elements per K block
constexpr int W = 8;              // waves per workgroup
constexpr int TILE_ROWS = 32 * W;
constexpr int TAU_SLOTS = 384;    // floats of LDS for the thresholds of the 320-query tile-subset kernel: lane (i, g) of query half qh
                                  // reads slots qh * 160 + (g + 4 j) * 16 + i, j = 0 .. 2 (at most 351)

// packed[kb][q][slot ^ ((q>>1)&7)] = 16-byte slot `slot` of K block kb of query q   (bn queries per tile)
// Query rows at or past n_rows (counted over all passes of the launch) are the padding of the last pass: they are packed as zeros, so
// the caller's [n_rows][d] array is read where it lies and needs no padded copy.
__global__ void pack_queries_kernel(const uint16_t* __restrict__ queries, int d, int bn, int n_rows, uint4* __restrict__ packed) {
    const int nkb = d / KB;
    const int QT_SLOTS = bn * 8;
    const int total = nkb * QT_SLOTS;
    queries += (size_t)blockIdx.y * bn * d;   // batched passes: pass y = the next bn query rows, the next `total` slots
    n_rows -= blockIdx.y * bn;
    packed += (size_t)blockIdx.y * total;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int kb = idx / QT_SLOTS;
        const int r = idx % QT_SLOTS;
        const int q = r >> 3, slot_sw = r & 7;
        const int slot = slot_sw ^ ((q >> 1) & 7);
        packed[idx] = q < n_rows ? *reinterpret_cast<const uint4*>(queries + (size_t)q * d + kb * KB + slot * 8) : uint4{0u, 0u, 0u, 0u};
    }
}

__device__ __forceinline__ half8 as_half8(const u32x4& v) { return __builtin_bit_cast(half8, v); }

// s_waitcnt vmcnt(N) placed by hand: the "memory" clobber keeps LDS reads below it, the sched_barrier keeps
// register-only MFMAs from being hoisted above it (cdna_hip_programming.md 5.4 rule 18).
template <int N> __device__ __forceinline__ void vm_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// one LDS-DMA instruction: 16 bytes per lane, LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void dma16(const void* gptr, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gptr,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Filtered search (include/mse.h mse_filter): the MASKED form of the scan kernels takes two trailing arguments, the filter's
// bitmap (one u32 word per 32-row group, bit r = row 32 g + r) and its word count (groups at or past it have no allowed row).  An
// accumulator of an excluded row enters its group's maximum as -FLT_MAX, so a group without allowed rows writes -FLT_MAX and every
// allowed row stays below its group's (masked) maximum: the certificate holds as it is.  The unmasked kernels take an empty pack,
// so their argument lists and code are those of the kernels before the masked form existed.
constexpr float MASKED_OUT = -3.402823466e+38f;
__device__ __forceinline__ uint32_t group_word(size_t group, const uint32_t* words, size_t n_words) {
    return group < n_words ? words[group] : 0u;
}

// S = stages in each wave's ring of X K-blocks (S-1 blocks in flight beyond the one being consumed);
// nkb must be a multiple of S so that stage indices are compile-time constants.
// NCT = 16-query column tiles per pass (8: 128 queries, 16: 256 queries)
// ABL (developer ablations, MSE_SCAN_ABL; results are then meaningless, only the timing is of interest):
// bit 0 no MFMAs, bit 1 no query-tile DMA, bit 2 no X DMA, bit 3 no B-fragment LDS reads
template <int S, int NCT, int ABL = 0, typename... Mask>
__global__ __launch_bounds__(W * 64) void scan_mfma_kernel(const uint16_t* __restrict__ base, size_t n_rows, int d,
                                                           const uint4* __restrict__ packed_ro,
                                                           float* __restrict__ gmax, int nq_pad, size_t n_tiles, uint32_t y_packed, uint32_t y_cols,
                                                           Mask... mask) {
    constexpr int BN = NCT * 16;
    constexpr int QT_BYTES = BN * 128;       // one query tile: BN x 64 f16
    constexpr int QI = BN / 64;              // DMA instructions per wave per query tile
    constexpr bool ILV = S >= 2 && !(ABL & 16);   // DMA pieces interleaved with the MFMA groups (ABL bit 4: burst, as in round 1)
    extern __shared__ __attribute__((aligned(16))) char smem[];  // ALL LDS in one object (5.x trap (a))
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int nkb = d / KB;
    const size_t row_bytes = (size_t)d * 2;
    const int swz = (i >> 1) & 7;
    const size_t n_groups = (n_rows + 31) / 32;
    char* const qbase = smem;                                     // [2][BN x 128 B] query tiles
    char* const xbase = smem + 2 * QT_BYTES + wave * (S * 4096);  // this wave's ring: S stages x 4 KiB
    gmax += (size_t)blockIdx.y * y_cols;   // batched passes (launch_scan_mfma n_pass > 1): pass y has its own query tiles and columns
    const char* const packed = reinterpret_cast<const char*>(packed_ro + (size_t)blockIdx.y * y_packed) + (size_t)(wave * QI * 64 + lane) * 16;

    size_t tile = blockIdx.x;
    if (tile >= n_tiles) return;

    // global source of this lane for DMA instruction u of a stage: row 8u + (lane>>3), piece (lane&7) ^ f(row).
    // Rows past the end are clamped to the last row: they only duplicate a row of the same (last) group.
    auto src_ptr = [&](size_t t, int u) -> const char* {
        const int r = 8 * u + (lane >> 3);
        size_t row = t * TILE_ROWS + wave * 32 + r;
        if (row >= n_rows) row = n_rows - 1;
        const int piece = (lane & 7) ^ ((r >> 1) & 7);
        return reinterpret_cast<const char*>(base) + row * row_bytes + piece * 16;
    };
    auto dma_x = [&](const char* (&rp)[4], int kblock, int stage) {
        char* dst = xbase + stage * 4096;
        if (ABL & 4) return;
#pragma unroll
        for (int u = 0; u < 4; u++) dma16(rp[u] + (size_t)kblock * 128, dst + u * 1024);
    };
    auto dma_q = [&](int kblock, int qb) {
        const char* src = packed + (size_t)kblock * QT_BYTES;
        char* dst = qbase + qb * QT_BYTES + wave * (QI * 1024);
        if (ABL & 2) return;
#pragma unroll
        for (int u = 0; u < QI; u++) dma16(src + u * 1024, dst + u * 1024);
    };

    const char* rp[4];
    const char* rn[4];
#pragma unroll
    for (int u = 0; u < 4; u++) rp[u] = src_ptr(tile, u);
    // prologue: query tile 0 and X blocks 0..S-2; drained completely so the counted waits start in steady state
    dma_q(0, 0);
#pragma unroll
    for (int j = 0; j < S - 1; j++) dma_x(rp, j % nkb, j);
    vm_wait<0>();
    __builtin_amdgcn_s_barrier();

    int buf = 0;
    while (true) {
        float4v acc[2][NCT];
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[rt][ct][r] = 0.0f;

        const size_t next_tile = tile + gridDim.x;
        const bool has_next_tile = next_tile < n_tiles;
#pragma unroll
        for (int u = 0; u < 4; u++) rn[u] = has_next_tile ? src_ptr(next_tile, u) : rp[u];

        for (int kb0 = 0; kb0 < nkb; kb0 += S) {
#pragma unroll
            for (int j = 0; j < S; j++) {
                const int kb = kb0 + j;
                // ---- DMA pieces of this iteration, always in this order: next query tile (QI), then the X block S-1 steps
                // ahead (4).  ILV: one piece at a time BETWEEN the MFMA groups below -- a burst of QI + 4 pieces at the top
                // costs each wave 100-185 cycles of issue per piece while both waves of the SIMD sit in the same phase and
                // the matrix core idles (measured: 256-query pass 5.94 ms burst vs MFMA-only 3.63 / DMA-only 4.58 at 1e7 rows).
                const int kq = kb + 1 == nkb ? 0 : kb + 1;
                const int kf = kb + S - 1;
                const bool x_next = kf >= nkb;                                 // first blocks of the next tile
                const size_t xoff = (size_t)(kf >= nkb ? kf - nkb : kf) * 128;
                char* const xdst = xbase + ((j + S - 1) % S) * 4096;
                const char* const qsrc = packed + (size_t)kq * QT_BYTES;
                char* const qdst = qbase + (buf ^ 1) * QT_BYTES + wave * (QI * 1024);
                auto issue_piece = [&](int p) {
                    if (p < QI) { if (!(ABL & 2)) dma16(qsrc + p * 1024, qdst + p * 1024); }
                    else if (!(ABL & 4)) dma16((x_next ? rn[p - QI] : rp[p - QI]) + xoff, xdst + (p - QI) * 1024);
                };
                if (!ILV) {
#pragma unroll
                    for (int p = 0; p < QI + 4; p++) issue_piece(p);
                    // the X block consumed now was issued S-1 iterations ago: everything issued after it may fly on.
                    // (DMAs return in order; the epilogue's stores share the counter and only make a wait stricter.)
                    vm_wait<(QI + 4) * (S - 1)>();
                } else if (S == 2) {
                    vm_wait<0>();   // the block consumed now was the last thing issued in the previous iteration
                }
                // ILV, S >= 3: the block consumed now was issued BEFORE the query pieces the previous iteration's closing
                // wait already covered, so it has landed.

                const u32x4* xs = reinterpret_cast<const u32x4*>(xbase + j * 4096) + i * 8;
                const u32x4* qt = reinterpret_cast<const u32x4*>(qbase + buf * QT_BYTES) + i * 8;
                const int slot_a = g ^ swz, slot_b = (4 + g) ^ swz;  // k step 0 / 1 of the K block
                // B fragments are software pipelined one column-tile pair ahead of the MFMAs that consume them
                u32x4 bq[2][2];
                bq[0][0] = qt[0 * 128 + slot_a];
                bq[0][1] = qt[1 * 128 + slot_a];
                const half8 a00 = as_half8(xs[slot_a]), a10 = as_half8(xs[128 + slot_a]);  // row tile 0 / 1, k step 0
                const half8 a01 = as_half8(xs[slot_b]), a11 = as_half8(xs[128 + slot_b]);  // k step 1
                constexpr int NCP = NCT / 2;   // column-tile pairs per k step
#pragma unroll
                for (int t = 0; t < 2 * NCP; t++) {  // t = ks*NCP + column-tile pair
                    const int ks = t / NCP, cp = t % NCP;
                    if (t + 1 < 2 * NCP) {
                        const int ks2 = (t + 1) / NCP, cp2 = (t + 1) % NCP;
                        if (!(ABL & 8)) {
                            bq[(t + 1) & 1][0] = qt[(cp2 * 2) * 128 + (ks2 ? slot_b : slot_a)];
                            bq[(t + 1) & 1][1] = qt[(cp2 * 2 + 1) * 128 + (ks2 ? slot_b : slot_a)];
                        } else {
                            bq[(t + 1) & 1][0] = bq[t & 1][1];
                            bq[(t + 1) & 1][1] = bq[t & 1][0];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // keep the reads for t+1 ahead of the MFMAs of t
                    if (ILV) {
                        // pieces spread evenly over the 2*NCP MFMA groups: piece p goes before group 1 + p*STEP
                        constexpr int STEP = (2 * NCP) / (QI + 4);
                        if (t >= 1 && (t - 1) % STEP == 0 && (t - 1) / STEP < QI + 4) {
                            issue_piece((t - 1) / STEP);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    const half8 a0 = ks ? a01 : a00;
                    const half8 a1 = ks ? a11 : a10;
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const half8 b = as_half8(bq[t & 1][e]);
                        const int ct = cp * 2 + e;
                        if (!(ABL & 1)) {
                            acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b, acc[0][ct], 0, 0, 0);
                            acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b, acc[1][ct], 0, 0, 0);
                        } else {
                            asm volatile("" ::"v"(b), "v"(a0), "v"(a1));
                        }
                    }
                }
                // next query tile: this wave's share has landed once only the 4 X DMAs issued after it remain;
                // the barrier then makes every wave's share visible to all.  It also separates this iteration's
                // reads of tile `buf` from the DMA that overwrites it two iterations later.
                vm_wait<4>();
                __builtin_amdgcn_s_barrier();
                buf ^= 1;
            }
        }

        // epilogue: per query column, max over this wave's 32 rows (2 row tiles x 4 accumulator rows x 4 lane groups)
        const size_t group = tile * W + wave;
        if constexpr (sizeof...(Mask) != 0) {
            // acc[rt][ct][r] of lane (i, g) holds row 16 rt + 4 g + r of the group (16x16x32 C layout; LDS row = wave row, dma_x)
            const uint32_t w = group_word(group, mask...) >> (4 * g);
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if ((w >> (16 * rt + r)) & 1u) continue;
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) acc[rt][ct][r] = MASKED_OUT;
                }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
            float m = fmaxf(fmaxf(acc[0][ct][0], acc[0][ct][1]), fmaxf(acc[0][ct][2], acc[0][ct][3]));
            m = fmaxf(m, fmaxf(fmaxf(acc[1][ct][0], acc[1][ct][1]), fmaxf(acc[1][ct][2], acc[1][ct][3])));
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            if (g == 0 && group < n_groups) gmax[group * (size_t)nq_pad + ct * 16 + i] = m;
        }

        if (!has_next_tile) break;
        tile = next_tile;
#pragma unroll
        for (int u = 0; u < 4; u++) rp[u] = rn[u];
    }
    vm_wait<0>();  // nothing may still be writing this workgroup's LDS when it is released
}


// Round 3: 2-D wave split of the 256-query pass.  The 8 waves form 4 row groups x 2 query halves; a wave owns 64 rows x 128
// queries (4 x 8 MFMA tiles, the same 128 accumulator registers).  Per K block a wave now reads 8 A + 16 B fragments from LDS
// (24 KiB) instead of 4 + 32 (36 KiB), and every B fragment feeds four MFMAs.  The two waves of a row group share one ring
// (S stages x 64 rows x 128 B); each DMAs the 32 rows of its own half.  No extra barrier: the wait + barrier that publishes
// the next query tile at the end of iteration kb also covers X block kb+1 (issued one iteration earlier, and older in the
// in-order vmcnt queue than the query pieces the wait is counted for).
// MF = 16: v_mfma_f32_16x16x32_f16; MF = 32: v_mfma_f32_32x32x16_f16 (2 x 4 tiles of 32 x 32, 16 accumulators each) over the
// same LDS images.
//
// BN = queries per pass: 256, or 320 (MF = 16, S = 2 only): a wave owns 64 rows x 160 queries (4 x 10 tiles, 160 accumulators) and
// reads 8 A + 20 B fragments per K block where the 1-D <2,20> kernel reads 4 + 40 for the same 80 MFMAs (224 against 352 KiB of LDS
// reads per K block per CU).  LDS: 2 x 40 KiB of query tiles + 4 row groups x 2 stages x 8 KiB = 144 KiB, as the 1-D kernel.
// The two-stage ring differs from the 1-D kernel's in one thing.  There a wave consumes only rows it fetched itself, so its own
// vmcnt(0) at the top of an iteration is enough.  Here half of the block a wave consumes next was fetched by its partner wave, and
// only a barrier AFTER the partner's wait publishes it: the closing wait of an iteration is vmcnt(0), not vmcnt(4), and nothing is
// waited for at the top.  Block kb + 1 and query tile kb + 1 are therefore both issued and landed inside iteration kb (their
// buffers are free from its first instruction: both were last read in iteration kb - 1, which ended in a barrier), and the row
// pieces, which come from HBM, go FIRST and close together (in front of MFMA groups 1, 2, 3, 4), the query pieces, L2 hits, after them
// (6, 8, .. 14), so that the last piece has six MFMA groups of flight before the closing wait.
// MEASURED (1e8 x 1152 rows, one process, arms alternated, six rounds of 3 s, profiles/scan_320_2d_ab.txt), scan kernel / queries/s:
// 1-D <2,20> 70.35 ms / 4 483 | this schedule 68.05 ms / 4 632 (+3.3 %, in every round) | rows first, a piece in front of every other
// group (1 .. 17; PROF = 5) 69.80 ms / 4 518 | queries first (PROF = 4) 73.08 ms / 4 317 against 70.73 / 4 459 for <2,20> on that box:
// with everything due inside one iteration, what is issued late is waited for.
// Code object: register and scratch figures at launch_scan_mfma's 320-query branch.  The masked form (filtered search) spills two
// registers with this order and keeps the every-other-group one.
//
// MID != 0 (the search kernel, GR = 64: plain, masked and tile-subset form): a row stage is recycled in the MIDDLE of the K block that
// consumes it, and rows are fetched two blocks ahead -- no more LDS, no more registers.
//   - Row block kb lives in stage kb & 1 (the K-block count is even).  The first tile's prologue fetches blocks 0 and 1, one into each
//     stage, and query tile 0; vmcnt(0); barrier.
//   - First half of iteration kb (MFMA groups t < NCTW, k step 0): the QI query pieces of tile kb + 1, in front of groups 0, 2, .. 8.
//     No row pieces.  The A fragments of k step 1 are read at ct == NCTW - 2 as before, so by group NCTW every read of the stage is issued.
//   - In front of group NCTW: s_waitcnt lgkmcnt(0) (those reads have returned), then a barrier, fenced for the scheduler on both
//     sides.  Behind it no wave of the workgroup reads stage kb & 1 again in this iteration.  Every wave reaches it: it hangs on a
//     constant of the unrolled loop, not on a lane or a wave, and the only early exit of the kernel is in front of the first barrier.
//   - Second half: the four row pieces of block kb + 2 into stage kb & 1, in front of groups NCTW + 1, + 3, + 5, + 7.  Past the end of
//     the tile, blocks nkb and nkb + 1 are blocks 0 and 1 of the workgroup's next tile (rn[]): a tile starts with its first two blocks
//     in LDS or in flight.  Behind its last tile rn[] repeats rp[]: two blocks land in stages nobody reads again, and the vmcnt(0) at
//     the end of the kernel waits for them.  (Fetching nothing there needs a uniform branch per piece and one at the closing wait;
//     with those in the K loop hipcc spills 60 to 80 registers.)
//   - Closing wait vmcnt(4), barrier.  A wave's loads and stores retire in order and the four youngest are the row pieces just
//     issued, so everything older has landed: this iteration's query pieces and this wave's half of block kb + 1 (issued in the second
//     half of iteration kb - 1); the partner's half is covered by the partner's own wait in front of the same barrier.  The epilogue's
//     stores and atomics lie between two tiles in that queue and only make a wait stricter.
// Rows get about 1.5 K blocks of flight instead of 0.85, query pieces 0.5 to 1 instead of at most 0.7.  The MFMAs, their order and their
// operands are the same, so every group maximum is bit-identical.  MEASURED (profiles/scan_midblock_prof.txt, scan_midblock_ab.txt): the
// closing vmcnt wait falls from 430-470 cycles per K block to 50, but most of that comes back at the two barriers and in the issue
// stretch (stamped cycles per K block: 3 205 -> 3 150 dense, 3 245 -> 3 225 thresholded); whole steps at 1e8 rows gain about 2 %.
//
// The turn-over between two row tiles of the search kernel (BN = 320, GR = 64: TURN; plain, masked and tile-subset form).  Between
// the last barrier of a tile and the first K block of the next all eight waves are in the same phase and no MFMA issues; the cycle
// stamps (PROF = 1, MSE_SCAN_ABL=33, profiles/scan_turnover_prof.txt) put that stretch at 8.3 % (dense) and 9.1 % (thresholded) of a
// tile's cycles with the epilogue this one replaced (a balanced fmaxf tree per column tile, two dependent ds_bpermute round trips per
// column tile, ten gated stores or append blocks, thresholds re-loaded from global memory, next-tile row pointers by a 64-bit multiply
// and a clamp per lane and piece, accumulators zeroed twice).  Now:
//   - a lane's maximum over its 16 rows of a column tile is one fmaxf chain (v_max3_f32);
//   - the maximum over the four 16-lane rows g is formed in registers and TRANSPOSED: v_permlane16_swap on the pairs of column
//     tiles (2 j, 2 j + 1) + one max: ten registers -> five; v_permlane32_swap on pairs of those + one max: five -> three.  No LDS,
//     no waits.  Afterwards lane (i, g) holds in register j the finished maximum of column i of column tile 4 j + g of its query half
//     (j = 0 .. 2; j = 2: g < 2 only; rows 2, 3 hold copies there and stay silent);
//   - dense: three stores per tile, each 16-lane row one whole 64-byte segment; thresholded: three compare-and-append blocks with
//     all 64 lanes eligible, thresholds read from a copy in LDS made once per workgroup (TAU_SLOTS).  The lists hold the same
//     (group, maximum) pairs and the arrays the same values as before; only who writes them changed;
//   - the next tile's row pointers are this tile's plus a distance the scalar unit works out, unless one of the two tiles is ragged;
//   - the K loop is entered without a test, so the accumulators are zeroed once.  (Not taken: the first k step on a constant-zero C
//     operand.  It needs a second copy of the first two K blocks, and hipcc spills 32 to 36 registers in that copy.)
typedef float float16v __attribute__((ext_vector_type(16)));

#ifdef MSE_DEV_KERNELS
// developer profile of the 2-D kernel (PROF = 1): shader cycles a wave spends [0] issuing a K block (barrier release -> closing wait),
// [1] in the closing vmcnt wait, [2] at the barrier; [3] = K blocks counted; [4] in the turn-over between the K loops of two row tiles
// (a tile's prologue, up to its first K block, and its epilogue, from its last closing barrier on), [5] = tiles counted, [6] at the
// mid-block barrier of the MID schedule (its lgkmcnt wait and the barrier; taken out of [0]).  s_memtime
// stamps sit where lgkmcnt is drained anyway.  MSE_SCAN_2D=161: the 256-query kernel; MSE_SCAN_ABL=33: the 320-query search kernel
// (64 rows per maximum), plain and tile-subset form.
__device__ unsigned long long g_scan_prof[7];
__device__ __forceinline__ uint32_t memtime() { return (uint32_t)__builtin_amdgcn_s_memtime(); }   // deltas fit 32 bits
#endif

// The trailing pack is empty (the plain kernel), the filter's bitmap and word count (the masked form), or one ScanSparse (the tile-subset
// form of the 320-query search pass, kernels.h): its tile map is three scalars, its epilogue dense or thresholded by a uniform branch.
template <typename... M> struct is_tile_subset : std::false_type {};
template <> struct is_tile_subset<ScanSparse> : std::true_type {};
template <typename... M> __device__ __forceinline__ ScanSparse tile_subset_of(const M&...) { return ScanSparse{}; }
__device__ __forceinline__ ScanSparse tile_subset_of(const ScanSparse& sp) { return sp; }

template <int S, int MF, int PROF = 0, int BN = 256, int GR = 32, int MID = 0, typename... Mask>
__global__ __launch_bounds__(W * 64) void scan_mfma2d_kernel(const uint16_t* __restrict__ base, size_t n_rows, int d,
                                                             const uint4* __restrict__ packed_ro,
                                                             float* __restrict__ gmax, int nq_pad, size_t n_tiles, uint32_t y_packed, uint32_t y_cols,
                                                             Mask... mask) {
    constexpr bool SPF = is_tile_subset<Mask...>::value;
    constexpr bool MASKED = sizeof...(Mask) != 0 && !SPF;
    static_assert(sizeof...(Mask) == 0 || (MF == 16 && (PROF == 0 || (PROF == 1 && is_tile_subset<Mask...>::value))),
                  "the masked form is the product kernel's");
    static_assert(!SPF || (BN == 320 && GR == 64), "a tile subset: the 320-query search pass only");
    static_assert(BN == 256 || (BN == 320 && MF == 16 && S == 2), "320 queries: 16x16x32 tiles on the two-stage ring only");
    static_assert(GR == 32 || (GR == 64 && MF == 16), "rows per written maximum: 32, or the wave's 64");
    static_assert(MID == 0 || (S == 2 && BN == 320 && (PROF == 0 || PROF == 1)), "the mid-block barrier: the two-stage ring of the 320-query kernel");
    constexpr int HALF = BN / 2;             // queries of one query half
    constexpr int QT_BYTES = BN * 128;
    constexpr int QI = BN / 64;              // DMA pieces per wave per query tile: 8 waves x QI x 64 lanes = the tile's BN x 8 slots
    constexpr bool XF = S == 2 && PROF != 4; // two-stage ring: row pieces FIRST (see the closing wait); PROF = 4: query pieces first;
                                             // PROF = 5: rows first, one piece in front of every other MFMA group as in the S = 3 form
    constexpr int CLOSE = S == 2 && !MID ? 0 : 4;   // DMAs that may still fly at the closing barrier (MID: the row pieces of block kb + 2)
    constexpr int RG_BYTES = 64 * 128;       // one K block of a row group
    constexpr bool TURN = BN == 320 && GR == 64;   // the search kernel's short turn-over between two row tiles (header comment)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    // (the search kernel has no register to spare for its epilogue's addressing: it keeps the wave index in a scalar)
    const int lane = tid & 63, wave = TURN ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int rg = wave >> 1, qh = wave & 1;
    const int nkb = d / KB;
    const size_t row_bytes = (size_t)d * 2;
    const size_t n_groups = (n_rows + GR - 1) / GR;
    char* const qbase = smem;
    char* const xbase = smem + 2 * QT_BYTES + rg * (S * RG_BYTES);
    gmax += (size_t)blockIdx.y * y_cols;   // batched passes (launch_scan_mfma n_pass > 1): pass y has its own query tiles and columns
    const char* const packed = reinterpret_cast<const char*>(packed_ro + (size_t)blockIdx.y * y_packed) + (size_t)(wave * QI * 64 + lane) * 16;

    // vt counts the tiles of this launch, tile is the base's: the same thing unless the launch covers a subset
    const ScanSparse sp = tile_subset_of(mask...);
    const size_t n_vt = SPF ? sp.n_tiles : n_tiles;
    auto tile_of = [&](size_t v) -> size_t { return SPF ? v * sp.mul + (v >> sp.shift) + sp.add : v; };
    size_t vt = blockIdx.x;
    if (vt >= n_vt) return;
    size_t tile = tile_of(vt);

    // this wave's DMA share of a K block: rows qh*32 + 8u + (lane>>3) of the row group, u = 0..3
    auto src_ptr = [&](size_t t, int u) -> const char* {
        const int r = qh * 32 + 8 * u + (lane >> 3);
        size_t row = t * TILE_ROWS + rg * 64 + r;
        if (row >= n_rows) row = n_rows - 1;
        const int piece = (lane & 7) ^ ((r >> 1) & 7);
        return reinterpret_cast<const char*>(base) + row * row_bytes + piece * 16;
    };
    const char* rp[4];
    const char* rn[4];
#pragma unroll
    for (int u = 0; u < 4; u++) rp[u] = src_ptr(tile, u);
    {
        char* qdst = qbase + wave * (QI * 1024);
#pragma unroll
        for (int u = 0; u < QI; u++) dma16(packed + u * 1024, qdst + u * 1024);
#pragma unroll
        for (int j = 0; j < (MID ? S : S - 1); j++)   // MID: blocks 0 and 1, one into each stage
#pragma unroll
            for (int u = 0; u < 4; u++) dma16(rp[u] + (size_t)(j % nkb) * 128, xbase + j * RG_BYTES + (qh * 4 + u) * 1024);
    }
    // tile-subset form, thresholded: the pass's thresholds, once per workgroup, behind the query tiles and the row rings (TAU_SLOTS
    // floats, launch_scan_mfma_tiles sizes the LDS); past the BN columns +inf, which no maximum exceeds
    float* const tau_lds = reinterpret_cast<float*>(smem + 2 * QT_BYTES + 4 * S * RG_BYTES);
    if constexpr (SPF) {
        if (sp.tau && tid < TAU_SLOTS) tau_lds[tid] = tid < BN ? sp.tau[tid] : __builtin_inff();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // written before the barrier below lets anyone read it
    }
    vm_wait<0>();
    __builtin_amdgcn_s_barrier();

    // fragment addressing: MF = 16: lane (i = lane & 15, g = lane >> 4): row / query i of a 16-tile, 16-byte k slot 4*ks + g;
    //                      MF = 32: lane (i = lane & 31, g = lane >> 5): row / query i of a 32-tile, k slot 2*ks + g (ks = 0..3)
    const int i = MF == 16 ? (lane & 15) : (lane & 31);
    const int g = MF == 16 ? (lane >> 4) : (lane >> 5);
    const int swz = (i >> 1) & 7;
    constexpr int NKS = MF == 16 ? 2 : 4;          // k steps per K block
    constexpr int NRT = 64 / MF, NCTW = HALF / MF; // row / column tiles of the wave
    constexpr int NACC = MF == 16 ? 4 : 16;
    typedef typename std::conditional<MF == 16, float4v, float16v>::type accv;

    int buf = 0;
#ifdef MSE_DEV_KERNELS
    uint32_t pt_issue = 0, pt_wait = 0, pt_bar = 0, pt_n = 0, pt_last = 0, pt_turn = 0, pt_tiles = 0, pt_mid = 0;
    if constexpr (PROF == 1) pt_last = memtime();
#endif
    while (true) {
        accv acc[NRT][NCTW];
#pragma unroll
        for (int rt = 0; rt < NRT; rt++)
#pragma unroll
            for (int ct = 0; ct < NCTW; ct++)
#pragma unroll
                for (int r = 0; r < NACC; r++) acc[rt][ct][r] = 0.0f;

        const size_t next_vt = vt + gridDim.x;
        const size_t next_tile = tile_of(next_vt);
        const bool has_next_tile = next_vt < n_vt;
        // TURN: both tiles whole (a uniform test; only the base's last tile can be ragged): the next tile's rows lie a wave-uniform
        // distance from this tile's, which the scalar unit works out -- no 64-bit multiply and no row clamp per lane and piece
        if (TURN && has_next_tile && (tile + 1) * TILE_ROWS <= n_rows && (next_tile + 1) * TILE_ROWS <= n_rows) {
            const size_t ahead = (next_tile - tile) * TILE_ROWS * row_bytes;
#pragma unroll
            for (int u = 0; u < 4; u++) rn[u] = rp[u] + ahead;
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++) rn[u] = has_next_tile ? src_ptr(next_tile, u) : rp[u];
        }

#ifdef MSE_DEV_KERNELS
        if constexpr (PROF == 1) {   // the prologue ends here: charged to the turn-over, not to the first K block
            // (the zeroed accumulators are made to exist here: left alone, hipcc zeroes them behind the stamp)
#pragma unroll
            for (int rt = 0; rt < NRT; rt++)
#pragma unroll
                for (int ct = 0; ct < NCTW; ct++) asm volatile("" : "+v"(acc[rt][ct]));
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t t = memtime();
            pt_turn += t - pt_last; pt_last = t;
            __builtin_amdgcn_sched_barrier(0);
        }
#endif
        // TURN: the loop is entered without a test (nkb >= S always: the launchers want a positive multiple).  With the test hipcc
        // zeroes the 160 accumulators twice per tile, once for the path around the loop and once for the loop
        for (int kb0 = 0; kb0 < nkb || (TURN && kb0 == 0); kb0 += S) {
#pragma unroll
            for (int j = 0; j < S; j++) {
                const int kb = kb0 + j;
                const int kq = kb + 1 == nkb ? 0 : kb + 1;
                const int kf = MID ? kb + 2 : kb + S - 1;   // the row block fetched in this iteration
                const bool x_next = kf >= nkb;
                const size_t xoff = (size_t)(kf >= nkb ? kf - nkb : kf) * 128;
                // MID: into the stage being consumed, behind the mid-block barrier.  (Behind its last tile a workgroup has nothing to
                // fetch; rn[] then repeats rp[] and the two blocks land in stages nobody reads again.  Skipping them takes a uniform
                // branch per piece and another at the closing wait, and with those hipcc spills 60 to 80 registers.)
                char* const xdst = xbase + (MID ? j : (j + S - 1) % S) * RG_BYTES + qh * 4096;
                const char* const qsrc = packed + (size_t)kq * QT_BYTES;
                char* const qdst = qbase + (buf ^ 1) * QT_BYTES + wave * (QI * 1024);
                auto issue_piece = [&](int p) {
                    const int pq = XF ? p - 4 : p, px = XF ? p : p - QI;
                    if (XF ? p >= 4 : p < QI) dma16(qsrc + pq * 1024, qdst + pq * 1024);
                    else dma16((x_next ? rn[px] : rp[px]) + xoff, xdst + px * 1024);
                };

                const u32x4* xs = reinterpret_cast<const u32x4*>(xbase + j * RG_BYTES) + i * 8;
                const u32x4* qt = reinterpret_cast<const u32x4*>(qbase + buf * QT_BYTES) + (qh * HALF + i) * 8;
                auto slot = [&](int ks) { return (MF == 16 ? (4 * ks + g) : (2 * ks + g)) ^ swz; };
                half8 a[2][NRT];   // A fragments of k step ks live in a[ks & 1]; the next k step's are read while this one multiplies
#pragma unroll
                for (int rt = 0; rt < NRT; rt++) a[0][rt] = as_half8(xs[rt * (MF * 8) + slot(0)]);
                constexpr int NT = NKS * NCTW;   // B fragments per K block: 16 at 256 queries in both forms, 20 at 320
                u32x4 bq[3];
                bq[0] = qt[0 * (MF * 8) + slot(0)];
                bq[1] = qt[1 * (MF * 8) + slot(0)];
#pragma unroll
                for (int t = 0; t < NT; t++) {   // t = ks * NCTW + ct
                    const int ks = t / NCTW, ct = t % NCTW;
                    if (t + 2 < NT) bq[(t + 2) % 3] = qt[((t + 2) % NCTW) * (MF * 8) + slot((t + 2) / NCTW)];
                    if (ct == NCTW - 2 && ks + 1 < NKS) {
#pragma unroll
                        for (int rt = 0; rt < NRT; rt++) a[(ks + 1) & 1][rt] = as_half8(xs[rt * (MF * 8) + slot(ks + 1)]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    // MID: the mid-block barrier.  The A fragments of both k steps have been read (ct == NCTW - 2 above) and the lgkmcnt
                    // wait retires them; behind the barrier no wave reads this row stage again before the closing barrier, so the row
                    // pieces of block kb + 2 may land in it.  Every wave reaches it: t is a constant of the unrolled loop
                    constexpr int MBAR = NCTW + (MID == 4 ? 1 : 0);
                    if constexpr (MID != 0) {
                        if (t == MBAR) {
#ifdef MSE_DEV_KERNELS
                            uint32_t m0 = 0;
                            if constexpr (PROF == 1) m0 = memtime();
#endif
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            __builtin_amdgcn_sched_barrier(0);
                            __builtin_amdgcn_s_barrier();
                            __builtin_amdgcn_sched_barrier(0);
#ifdef MSE_DEV_KERNELS
                            if constexpr (PROF == 1) {
                                pt_mid += memtime() - m0;
                                __builtin_amdgcn_sched_barrier(0);
                            }
#endif
                        }
                    }
                    {
                        constexpr int STEP = NT / (QI + 4);
                        int pc = -1;   // the DMA piece issued in front of MFMA group t (t is a constant of the unrolled loop)
                        // MID: query pieces in the first half (in front of groups 0, 2, .. 8), row pieces behind the mid-block barrier:
                        // MID = 2 (the product's) in front of groups NCTW + 1, + 3, + 5, + 7; MID = 1 in front of NCTW .. NCTW + 3.
                        // Two more developer placements: MID = 3 as 1 with the queries in front of groups 1 .. 5; MID = 4 as 1 with the
                        // barrier and the rows one group later
                        if constexpr (MID != 0) {
                            if (t < NCTW) {
                                if (MID == 3 ? (t >= 1 && t <= QI) : (t % 2 == 0 && t / 2 < QI)) pc = 4 + (MID == 3 ? t - 1 : t / 2);
                            } else if (MID == 2) {
                                if ((t - MBAR) % 2 == 1 && (t - MBAR) / 2 < 4) pc = (t - MBAR) / 2;
                            } else if (t >= MBAR && t - MBAR < 4) pc = t - MBAR;
                        } else
                        // row pieces before groups 1-4, query pieces before 6, 8, ...; the masked form keeps the every-other-group
                        // order of PROF = 5: with the early order it spills two registers (12 B of scratch)
                        if constexpr (S == 2 && PROF != 4 && PROF != 5 && !MASKED) {
                            if (t >= 1 && t <= 4) pc = t - 1;
                            else if (t >= 6 && (t - 6) % 2 == 0 && (t - 6) / 2 < QI) pc = 4 + (t - 6) / 2;
                        } else if (t >= 1 && (t - 1) % STEP == 0 && (t - 1) / STEP < QI + 4) pc = (t - 1) / STEP;
                        if (pc >= 0) {
                            issue_piece(pc);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    const half8 b = as_half8(bq[t % 3]);
                    if constexpr (PROF == 3) __builtin_amdgcn_s_setprio(1);   // developer variant: MFMA groups at raised issue priority
#pragma unroll
                    for (int rt = 0; rt < NRT; rt++) {
                        if constexpr (MF == 16) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks & 1][rt], b, acc[rt][ct], 0, 0, 0);
                        else acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks & 1][rt], b, acc[rt][ct], 0, 0, 0);
                    }
                    if constexpr (PROF == 3) __builtin_amdgcn_s_setprio(0);
                }
#ifdef MSE_DEV_KERNELS
                if constexpr (PROF == 1) {
                    const uint32_t t0 = memtime();
                    vm_wait<CLOSE>();
                    const uint32_t t1 = memtime();
                    __builtin_amdgcn_s_barrier();
                    const uint32_t t2 = memtime();
                    pt_issue += t0 - pt_last; pt_wait += t1 - t0; pt_bar += t2 - t1; pt_n++; pt_last = t2;
                } else
#endif
                {
                    // MID: the CLOSE youngest loads are the row pieces of block kb + 2, issued behind the mid-block barrier of every
                    // iteration; everything older -- this iteration's query pieces, the rows of block kb + 1 -- has landed
                    vm_wait<CLOSE>();
#ifdef MSE_DEV_KERNELS
                    if constexpr (PROF != 2)   // PROF = 2: timing ablation WITHOUT the barrier (racy, results meaningless)
#endif
                    __builtin_amdgcn_s_barrier();
                }
                buf ^= 1;
            }
        }

        // epilogue: per query column, max over each 32-row group of this wave (two groups), or over all 64 rows (GR = 64)
        if constexpr (MASKED && GR == 32) {
            // acc[2 p + h][ct][r] of lane (i, g) holds row 16 h + 4 g + r of group p (LDS row = row of the row group, src_ptr)
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const uint32_t w = group_word(tile * W + rg * 2 + p, mask...) >> (4 * g);
#pragma unroll
                for (int h = 0; h < 2; h++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if ((w >> (16 * h + r)) & 1u) continue;
#pragma unroll
                        for (int ct = 0; ct < NCTW; ct++) acc[2 * p + h][ct][r] = MASKED_OUT;
                    }
            }
        }
        if constexpr (GR == 64) {
            // one maximum per wave and column: the wave's 64 rows are rows 64 (4 tile + rg) .. + 63 of the base.  Rows past the end were
            // clamped to the last row, which lies in the same 64-row group whenever that group has a row at all.
            const size_t group = tile * 4 + rg;
            // masked form: bit 4 rt + r of `allowed` = this lane's row 16 rt + 4 g + r of the wave (acc[rt][.][r]) is an allowed row; an
            // excluded row enters the maximum as MASKED_OUT (selected here, not written into the accumulators: that form spills)
            uint32_t allowed = 0xFFFFu;
            if constexpr (MASKED) {
                const uint32_t w0 = group_word(group * 2, mask...) >> (4 * g), w1 = group_word(group * 2 + 1, mask...) >> (4 * g);
                allowed = (w0 & 15u) | ((w0 >> 16 & 15u) << 4) | ((w1 & 15u) << 8) | ((w1 >> 16 & 15u) << 12);
            }
            auto av = [&](int rt, int ct, int r) {
                if constexpr (MASKED) return (allowed >> (4 * rt + r)) & 1u ? acc[rt][ct][r] : MASKED_OUT;
                else return acc[rt][ct][r];
            };
            static_assert(NCTW == 10, "the transposed reduction below is laid out for the ten column tiles of the 320-query kernel");
            uint32_t cbase = (uint32_t)(qh * HALF + i);   // this lane's column of column tile 0
            // opaque: everything addressed from it is worked out here, in the epilogue -- hoisted out of the tile loop, the list and
            // array offsets of a lane would have to live through the main loop, which has no register to spare
            asm volatile("" : "+v"(cbase));
            // this lane's maximum over its 16 rows of each column tile: one chain per tile, which hipcc folds into v_max3_f32 (the
            // balanced tree of fmaxf it replaced cost a canonicalising v_max per accumulator on top of its eleven)
            float m[NCTW];
#pragma unroll
            for (int ct = 0; ct < NCTW; ct++) {
                float x = av(0, ct, 0);
#pragma unroll
                for (int e = 1; e + 1 < 16; e += 2) x = fmaxf(fmaxf(x, av(e >> 2, ct, e & 3)), av((e + 1) >> 2, ct, (e + 1) & 3));
                m[ct] = fmaxf(x, av(3, ct, 3));
            }
            // Across the four 16-lane rows g, in registers and transposed.  v_permlane16_swap a, b exchanges rows 1, 3 of a with rows
            // 0, 2 of b, so max(a', b') holds in rows 0, 2 a's maximum over rows {0, 1}, {2, 3} and in rows 1, 3 b's: ten registers
            // become five.  v_permlane32_swap a, b exchanges rows 2, 3 of a with rows 0, 1 of b, so max(a', b') holds in rows 0, 1 the
            // finished maxima of a's two column tiles and in rows 2, 3 those of b's: five become three (the fifth pairs with itself).
            // Afterwards lane (i, g) holds in q[j] the maximum over the wave's 64 rows of column i of column tile 4 j + g (q[2]: g < 2).
            auto swap_max = [](float a, float b, auto half) {
                uint32_t ua = __builtin_bit_cast(uint32_t, a), ub = __builtin_bit_cast(uint32_t, b);
                uint32_t r0, r1;
                if constexpr (decltype(half)::value) {
                    const auto r = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
                    r0 = r[0]; r1 = r[1];
                } else {
                    const auto r = __builtin_amdgcn_permlane16_swap(ua, ub, false, false);
                    r0 = r[0]; r1 = r[1];
                }
                return fmaxf(__builtin_bit_cast(float, r0), __builtin_bit_cast(float, r1));
            };
            float p[5], q[3];
#pragma unroll
            for (int j = 0; j < 5; j++) p[j] = swap_max(m[2 * j], m[2 * j + 1], std::false_type{});
            q[0] = swap_max(p[0], p[1], std::true_type{});
            q[1] = swap_max(p[2], p[3], std::true_type{});
            q[2] = swap_max(p[4], p[4], std::true_type{});
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const uint32_t col = cbase + (4 * j + g) * MF;   // the column q[j] belongs to
                const bool mine = (j < 2 || g < 2) && group < n_groups;
#ifdef MSE_DEV_KERNELS
                if constexpr (PROF == 6) { asm volatile("" ::"v"(q[j])); continue; }   // timing ablation: the maxima are formed and not stored
#endif
                if constexpr (SPF) {
                    if (sp.tau) {
                        // thresholded: the few maxima above the column's threshold (read from the workgroup's copy in LDS) go to the
                        // column's list, nothing else is written.  All 64 lanes speak, each for its own column tiles
                        if (mine && q[j] > tau_lds[col]) {
                            uint32_t one;
                            asm volatile("v_mov_b32 %0, 1" : "=v"(one));   // made here, not kept in a register through the main loop
                            const uint32_t pos = atomicAdd(&sp.counts[col], one);
                            if (pos < sp.cap) {
                                sp.ids[col * sp.cap + pos] = (uint32_t)group;
                                sp.keys[col * sp.cap + pos] = q[j];
                            }
                        }
                    } else if (mine) {
                        gmax[(vt * 4 + rg) * (size_t)nq_pad + col] = q[j];   // the launch's own groups: a small dense array
                    }
                } else if (mine) {
                    gmax[group * (size_t)nq_pad + col] = q[j];   // four whole 64-byte segments per store, one per 16-lane row
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const size_t group = tile * W + rg * 2 + p;
#pragma unroll
                for (int ct = 0; ct < NCTW; ct++) {
                    float m;
                    if constexpr (MF == 16) {
                        m = fmaxf(fmaxf(acc[2 * p][ct][0], acc[2 * p][ct][1]), fmaxf(acc[2 * p][ct][2], acc[2 * p][ct][3]));
                        m = fmaxf(m, fmaxf(fmaxf(acc[2 * p + 1][ct][0], acc[2 * p + 1][ct][1]), fmaxf(acc[2 * p + 1][ct][2], acc[2 * p + 1][ct][3])));
                        m = fmaxf(m, __shfl_xor(m, 16));
                        m = fmaxf(m, __shfl_xor(m, 32));
                    } else {
                        m = acc[p][ct][0];
#pragma unroll
                        for (int r = 1; r < 16; r++) m = fmaxf(m, acc[p][ct][r]);
                        m = fmaxf(m, __shfl_xor(m, 32));
                    }
                    if (g == 0 && group < n_groups) gmax[group * (size_t)nq_pad + qh * HALF + ct * MF + i] = m;
                }
            }
        }

#ifdef MSE_DEV_KERNELS
        if constexpr (PROF == 1) {   // the epilogue is charged to the turn-over, not to the next K block
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t t = memtime();
            pt_turn += t - pt_last; pt_last = t; pt_tiles++;
            __builtin_amdgcn_sched_barrier(0);
        }
#endif
        if (!has_next_tile) break;
        vt = next_vt;
        tile = next_tile;
#pragma unroll
        for (int u = 0; u < 4; u++) rp[u] = rn[u];
    }
    vm_wait<0>();
#ifdef MSE_DEV_KERNELS
    if constexpr (PROF == 1) {
        if (lane == 0) {
            atomicAdd(&g_scan_prof[0], (unsigned long long)(pt_issue - pt_mid)); atomicAdd(&g_scan_prof[1], (unsigned long long)pt_wait);
            atomicAdd(&g_scan_prof[2], (unsigned long long)pt_bar); atomicAdd(&g_scan_prof[3], (unsigned long long)pt_n);
            atomicAdd(&g_scan_prof[4], (unsigned long long)pt_turn); atomicAdd(&g_scan_prof[5], (unsigned long long)pt_tiles);
            if constexpr (MID != 0) atomicAdd(&g_scan_prof[6], (unsigned long long)pt_mid);
        }
    }
#endif
}


#ifdef MSE_DEV_KERNELS
// Round 3, third form: the 2-D tiling with the DMA ISSUE specialised by wave.  Waves 0-3 issue all row traffic (wave j streams the
// 64 rows of row group j: 8 pieces per K block), waves 4-7 all query-tile traffic (8 pieces each).  Every wave still multiplies its
// 64 x 128 tile.  Why: a wave's loads retire in order, so in the mixed form the closing wait for the next query tile (L2 hits
// issued a few hundred cycles ago) is also a wait for the row pieces in front of them, which pins the row prefetch to ~1.25 K blocks
// of flight time.  A row wave's queue holds only row pieces: block kb+2 is issued from the START of iteration kb and must land by
// the end of iteration kb+1 (~1.9 K blocks of flight), with the same 3-stage ring; a query wave's queue holds only L2 hits.
// Addresses: per lane two 64-bit pointers per tile (row lane>>3 of the row group, even / odd piece swizzle); a piece adds a
// wave-uniform offset (8u rows + the K block).  Needs n_rows % 256 == 0: the launcher sends a ragged tail through scan_mfma_kernel.
// MEASURED (1e7 rows, same box, answers equal the exact-order kernel): 5.98-6.01 ms against 5.59-5.60 ms for the mixed 2-D form --
// the pass is not bound by the flight time of the row prefetch.  Kept in the developer library only.

template <int S>
__global__ __launch_bounds__(W * 64) void scan_mfma2s_kernel(const uint16_t* __restrict__ base, size_t n_rows, int d,
                                                             const uint4* __restrict__ packed_ro,
                                                             float* __restrict__ gmax, int nq_pad, size_t n_tiles, uint32_t y_packed, uint32_t y_cols) {
    static_assert(S == 3, "the specialised schedule is written for the 3-stage ring");
    constexpr int BN = 256;
    constexpr int QT_BYTES = BN * 128;
    constexpr int RG_BYTES = 64 * 128;
    constexpr int NP = 8;                    // DMA pieces per wave per K block (rows: 64 x 128 B; queries: 1/4 of the 32 KiB tile)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg = wave >> 1, qh = wave & 1;
    const bool row_wave = wave < 4;          // wave-uniform
    const int w4 = wave & 3;
    const int nkb = d / KB;
    const size_t row_bytes = (size_t)d * 2;
    char* const qbase = smem;
    char* const xring = smem + 2 * QT_BYTES;                      // [4 row groups][S][8 KiB]
    char* const xbase = xring + rg * (S * RG_BYTES);              // the ring this wave READS
    char* const xfill = xring + w4 * (S * RG_BYTES);              // the ring a row wave FILLS (row group = wave)
    char* const qfill = qbase + w4 * (NP * 1024);                 // a query wave's quarter of a query tile
    gmax += (size_t)blockIdx.y * y_cols;
    const char* const packed = reinterpret_cast<const char*>(packed_ro + (size_t)blockIdx.y * y_packed) + (size_t)w4 * (NP * 1024) + lane * 16;

    size_t tile = blockIdx.x;
    if (tile >= n_tiles) return;

    // row wave j, piece u: row 8u + (lane >> 3) of row group j, 16-byte piece (lane & 7) ^ f(row), f(r) = (r >> 1) & 7 =
    // ((lane >> 4) + 4 (u & 1)) & 7: the odd pieces' lane offset is the even one with bit 6 flipped (row_bytes is a multiple of 128)
    const size_t lane_off = (size_t)(lane >> 3) * row_bytes + (size_t)(((lane & 7) ^ (lane >> 4)) * 16);
    const char* const rows0 = reinterpret_cast<const char*>(base) + (size_t)w4 * 64 * row_bytes;
    auto tile_ptr = [&](size_t t) { return rows0 + t * TILE_ROWS * row_bytes + lane_off; };
    const char* lp = tile_ptr(tile);   // even pieces; odd pieces: the same address with bit 6 flipped
    const char* ln = lp;
    const size_t piece_rows = 8 * row_bytes;
    auto dma_row_piece = [&](const char* p, int u, size_t koff, char* dst) {
        const char* q = (u & 1) ? reinterpret_cast<const char*>(reinterpret_cast<uintptr_t>(p) ^ 64u) : p;
        dma16(q + (u * piece_rows + koff), dst + u * 1024);
    };
    if (row_wave) {
#pragma unroll
        for (int j = 0; j < S - 1; j++)
#pragma unroll
            for (int u = 0; u < NP; u++) dma_row_piece(lp, u, (size_t)(j % nkb) * 128, xfill + j * RG_BYTES);
    } else {
#pragma unroll
        for (int u = 0; u < NP; u++) dma16(packed + u * 1024, qfill + u * 1024);
    }
    vm_wait<0>();
    __builtin_amdgcn_s_barrier();

    const int i = lane & 15, g = lane >> 4;
    const int swz = (i >> 1) & 7;
    int buf = 0;
    while (true) {
        float4v acc[4][8];
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < 8; ct++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[rt][ct][r] = 0.0f;

        const size_t next_tile = tile + gridDim.x;
        const bool has_next_tile = next_tile < n_tiles;
        ln = has_next_tile ? tile_ptr(next_tile) : lp;   // the last tile re-reads its own first blocks

        for (int kb0 = 0; kb0 < nkb; kb0 += S) {
#pragma unroll
            for (int j = 0; j < S; j++) {
                const int kb = kb0 + j;
                const int kq = kb + 1 == nkb ? 0 : kb + 1;
                const int kf = kb + S - 1;
                const char* const xp = kf >= nkb ? ln : lp;
                const size_t xoff = (size_t)(kf >= nkb ? kf - nkb : kf) * 128;
                char* const xdst = xfill + ((j + S - 1) % S) * RG_BYTES;
                const char* const qsrc = packed + (size_t)kq * QT_BYTES;
                char* const qdst = qfill + (buf ^ 1) * QT_BYTES;
                auto issue_piece = [&](int p) {
                    if (row_wave) dma_row_piece(xp, p, xoff, xdst);
                    else dma16(qsrc + p * 1024, qdst + p * 1024);
                };

                const u32x4* xs = reinterpret_cast<const u32x4*>(xbase + j * RG_BYTES) + i * 8;
                const u32x4* qt = reinterpret_cast<const u32x4*>(qbase + buf * QT_BYTES) + (qh * 128 + i) * 8;
                auto slot = [&](int ks) { return (4 * ks + g) ^ swz; };
                half8 a[2][4];
#pragma unroll
                for (int rt = 0; rt < 4; rt++) a[0][rt] = as_half8(xs[rt * 128 + slot(0)]);
                u32x4 bq[3];
                bq[0] = qt[0 * 128 + slot(0)];
                bq[1] = qt[1 * 128 + slot(0)];
#pragma unroll
                for (int t = 0; t < 16; t++) {   // t = ks * 8 + ct
                    const int ks = t / 8, ct = t % 8;
                    if (t + 2 < 16) bq[(t + 2) % 3] = qt[((t + 2) % 8) * 128 + slot((t + 2) / 8)];
                    if (ct == 6 && ks == 0) {
#pragma unroll
                        for (int rt = 0; rt < 4; rt++) a[1][rt] = as_half8(xs[rt * 128 + slot(1)]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (t >= 1 && (t - 1) % 2 == 0 && (t - 1) / 2 < NP) {
                        issue_piece((t - 1) / 2);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const half8 b = as_half8(bq[t % 3]);
#pragma unroll
                    for (int rt = 0; rt < 4; rt++) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ks][rt], b, acc[rt][ct], 0, 0, 0);
                }
                // row wave: everything but the 8 pieces of block kb+2 just issued has landed -> block kb+1 is in LDS;
                // query wave: tile kb+1 complete.  The barrier publishes both to all waves.
                if (row_wave) vm_wait<NP>(); else vm_wait<0>();
                __builtin_amdgcn_s_barrier();
                buf ^= 1;
            }
        }

#pragma unroll
        for (int p = 0; p < 2; p++) {
            const size_t group = tile * W + rg * 2 + p;
#pragma unroll
            for (int ct = 0; ct < 8; ct++) {
                float m = fmaxf(fmaxf(acc[2 * p][ct][0], acc[2 * p][ct][1]), fmaxf(acc[2 * p][ct][2], acc[2 * p][ct][3]));
                m = fmaxf(m, fmaxf(fmaxf(acc[2 * p + 1][ct][0], acc[2 * p + 1][ct][1]), fmaxf(acc[2 * p + 1][ct][2], acc[2 * p + 1][ct][3])));
                m = fmaxf(m, __shfl_xor(m, 16));
                m = fmaxf(m, __shfl_xor(m, 32));
                if (g == 0) gmax[group * (size_t)nq_pad + qh * 128 + ct * 16 + i] = m;
            }
        }
        if (!has_next_tile) break;
        tile = next_tile;
        lp = ln;
    }
    vm_wait<0>();
}
#endif  // MSE_DEV_KERNELS

// batched passes of one launch_scan_mfma call (set by it around its launches; launch_scan_mfma is not re-entered concurrently with
// different values on one thread: thread_local)
thread_local unsigned g_pass_count = 1;
thread_local uint32_t g_pass_packed = 0, g_pass_cols = 0;

template <typename K, typename... Mask>
int launch_kernel(K kernel, size_t lds, size_t grid, hipStream_t stream, const uint16_t* base, size_t n_rows, int d,
                  const uint4* packed, float* group_max, int nq_pad, Mask... mask) {
    const size_t n_tiles = (n_rows + TILE_ROWS - 1) / TILE_ROWS;
    if (grid > n_tiles) grid = n_tiles;
    MSE_DYN_LDS(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid, g_pass_count), dim3(W * 64), lds, stream, base, n_rows, d, packed, group_max, nq_pad, n_tiles,
                       g_pass_packed, g_pass_cols, mask...);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

template <int S, int NCT, int ABL, typename... Mask>
int launch_variant(size_t grid, hipStream_t stream, const uint16_t* base, size_t n_rows, int d, const uint4* packed,
                   float* group_max, int nq_pad, Mask... mask) {
    const size_t lds = 2 * (size_t)(NCT * 16 * 128) + (size_t)W * S * 4096;  // S = 3: 128 KiB at 128 queries, 160 KiB at 256
    return launch_kernel(scan_mfma_kernel<S, NCT, ABL, Mask...>, lds, grid, stream, base, n_rows, d, packed, group_max, nq_pad, mask...);
}

#ifdef MSE_DEV_KERNELS

template <int S>
int launch_2s(size_t grid, hipStream_t stream, const uint16_t* base, size_t n_rows, int d, const uint4* packed,
              float* group_max, int nq_pad) {
    const size_t lds = 2 * (size_t)(256 * 128) + (size_t)4 * S * 8192;
    const size_t n_full = n_rows / TILE_ROWS * TILE_ROWS;
    if (n_full && launch_kernel(scan_mfma2s_kernel<S>, lds, grid, stream, base, n_full, d, packed, group_max, nq_pad)) return -1;
    if (n_full < n_rows)   // ragged tail (< 256 rows): one workgroup of the row-clamping kernel
        return launch_variant<S, 16, 0>(1, stream, base + n_full * (size_t)d, n_rows - n_full, d, packed,
                                        group_max + (n_full / 32) * (size_t)nq_pad, nq_pad);
    return 0;
}
#endif

template <int S, int MF, int PROF = 0, int BN = 256, int GR = 32, int MID = 0, typename... Mask>
int launch_2d(size_t grid, hipStream_t stream, const uint16_t* base, size_t n_rows, int d, const uint4* packed,
              float* group_max, int nq_pad, Mask... mask) {
    const size_t lds = 2 * (size_t)(BN * 128) + (size_t)4 * S * 8192;   // 160 KiB at 256 queries (S = 3), 144 KiB at 320 (S = 2)
    return launch_kernel(scan_mfma2d_kernel<S, MF, PROF, BN, GR, MID, Mask...>, lds, grid, stream, base, n_rows, d, packed, group_max, nq_pad, mask...);
}

// The schedule of the 320-query search kernels (scan_mfma2d_kernel, MID; 64 rows per maximum: plain, masked and tile-subset form alike):
// the mid-block barrier and row blocks two ahead, the row pieces in front of every other MFMA group of the second half (MID = 2, the
// best of the four placements measured: profiles/scan_midblock_prof.txt, scan_midblock_ab.txt).  0 = the schedule before it, in which
// everything an iteration issues lands inside it; the 32-row forms keep that one (their masked form spills four registers with MID).
constexpr int MID_320 = 2;
#ifdef MSE_DEV_KERNELS
// developer library: MSE_SCAN_MID=0 .. 4 selects the schedule of the unmasked 64-row forms (0 the one before, 1, 3, 4 the other placements)
int dev_scan_mid() {
    const int m = getenv("MSE_SCAN_MID") ? atoi(getenv("MSE_SCAN_MID")) : MID_320;
    return m >= 0 && m <= 4 ? m : MID_320;
}
#endif

}  // namespace

// largest pass: 320 queries on the two-stage ring (the K-block count must be even), else 256
int mfma_query_tile(int d) { return (d / KB) % 2 == 0 ? 320 : 256; }
// padded query count of a pass of nq queries: 128, 192 (three-stage ring only: the K-block count must divide by 3) or 256
int mfma_pad(int nq, int d) {
    if (nq <= 128) return 128;
    if (nq <= 192 && (d / KB) % 3 == 0) return 192;
    if (nq <= 256 || (d / KB) % 2 != 0) return 256;
    return 320;
}

size_t mfma_packed_bytes(int d) { return (size_t)(d / KB) * 320 * 128; }

// rows per group maximum of a pass padded to nq_pad queries: the 320-query kernel's waves own 64 rows each and write one maximum for
// them; every other kernel writes 32-row groups.  (The developer library keeps 32 while one of its kernel knobs is set: the kernels
// they select write 32-row groups.)  -DMSE_GROUP_ROWS_320=32 builds the library with 32-row groups everywhere, for an A/B of the group
// size alone (scripts/step_tail_ab.py compares builds).
#ifndef MSE_GROUP_ROWS_320
#define MSE_GROUP_ROWS_320 64
#endif
int mfma_group_rows(int nq_pad) {
#ifdef MSE_DEV_KERNELS
    // MSE_SCAN_ABL=32 is the ablation of the 64-row form itself (no stores of group maxima), 33 its cycle profile: they keep its groups
    if (getenv("MSE_SCAN_2D") || (getenv("MSE_SCAN_ABL") && atoi(getenv("MSE_SCAN_ABL")) != 32 && atoi(getenv("MSE_SCAN_ABL")) != 33)) return 32;
#endif
    return nq_pad == 320 ? MSE_GROUP_ROWS_320 : 32;
}

// packed_scratch: mfma_packed_bytes(d) bytes of device scratch owned by the caller (per searcher)
int launch_scan_mfma(const uint16_t* base, size_t n_rows, int d, const uint16_t* queries_dev, int nq_pad,
                     void* packed_scratch, float* group_max, int n_cu, hipStream_t stream, hipEvent_t ev_begin,
                     hipEvent_t ev_end, int gm_stride, int n_pass, const uint32_t* mask, size_t mask_words, int nq_rows, int group_rows) {
    if (n_rows == 0) return 0;
    if (group_rows != 32 && !(group_rows == 64 && nq_pad == 320)) return fail("scan_mfma: 32 rows per group maximum, or 64 on the 320-query pass");
    if (nq_rows < 0) nq_rows = n_pass * nq_pad;
    if (n_pass < 1 || n_pass > 65535) return fail("scan_mfma: 1..65535 passes per launch");
    if (n_pass > 1 && !gm_stride) return fail("scan_mfma: batched passes need a common group-maximum stride");
    // the kernels use their last integer argument only as the row stride of group_max: a pass may write its nq_pad columns into a
    // wider array (several passes side by side, api.hip mfma_pass over a small base)
    const int gs = gm_stride ? gm_stride : nq_pad;
    if (gs < nq_pad) return fail("scan_mfma: group-maximum stride below the pass width");
    if (d % 64 != 0 || d <= 0 || d > D_MAX) return fail("vector width must be a positive multiple of 64");
    if (nq_pad != 128 && nq_pad != 256 && !(nq_pad == 192 && (d / KB) % 3 == 0) && !(nq_pad == 320 && (d / KB) % 2 == 0))
        return fail("scan_mfma: query tile must be padded to 128, 192 (K blocks divisible by 3), 256 or 320 (K blocks even)");
    uint4* packed = reinterpret_cast<uint4*>(packed_scratch);
    // n_pass > 1: queries_dev holds n_pass x nq_pad rows, packed_scratch n_pass x mfma_packed_bytes(d), and pass y writes columns
    // [y * nq_pad, (y + 1) * nq_pad) of group_max -- ONE launch; a small base (a few row tiles) then fills the chip with its passes
    // side by side instead of running them one after the other on a few CUs
    hipLaunchKernelGGL(pack_queries_kernel, dim3(64, (unsigned)n_pass), dim3(256), 0, stream, queries_dev, d, nq_pad, nq_rows, packed);
    struct PassScope {
        PassScope(unsigned n, uint32_t pk, uint32_t cols) { g_pass_count = n; g_pass_packed = pk; g_pass_cols = cols; }
        ~PassScope() { g_pass_count = 1; g_pass_packed = 0; g_pass_cols = 0; }
    } pass_scope((unsigned)n_pass, (uint32_t)((size_t)(d / KB) * nq_pad * 8), (uint32_t)nq_pad);
    if (ev_begin) MSE_HIP_TRY(hipEventRecord(ev_begin, stream));
    const int nkb = d / KB;
    const int S = nkb % 3 == 0 ? 3 : nkb % 2 == 0 ? 2 : 1;   // ring depth: 3 when the K-block count allows it
    const size_t grid = (size_t)n_cu;  // one workgroup per CU
    int rc = -2;
#ifdef MSE_DEV_KERNELS
    if (!mask && group_rows == 32) {
    // Developer build only (make dev -> libmse_hip_dev.so, scripts/scan_ablate.py): timing ablations whose RESULTS ARE WRONG
    // and alternative tilings.  None of this is compiled into the product library.
    const int abl = getenv("MSE_SCAN_ABL") ? atoi(getenv("MSE_SCAN_ABL")) : 0;
    const int v2d = getenv("MSE_SCAN_2D") ? atoi(getenv("MSE_SCAN_2D")) : -1;
    if (nq_pad == 128 && S == 3 && abl == 16) rc = launch_variant<3, 8, 16>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && abl) {   // timing ablations of the round-2 kernel
        switch (abl) {
            case 1: rc = launch_variant<3, 16, 1>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 2: rc = launch_variant<3, 16, 2>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 4: rc = launch_variant<3, 16, 4>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 6: rc = launch_variant<3, 16, 6>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 8: rc = launch_variant<3, 16, 8>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 9: rc = launch_variant<3, 16, 9>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 14: rc = launch_variant<3, 16, 14>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 16: rc = launch_variant<3, 16, 16>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            default: break;
        }
    }
    // the 320-query pass on the one-dimensional wave split (the product kernel of rounds 4-6) and the 2-D form's other piece orders
    else if (nq_pad == 320 && v2d == 0) rc = launch_variant<2, 20, 0>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 320 && v2d == 165) rc = launch_2d<2, 16, 5, 320>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 320 && v2d == 164) rc = launch_2d<2, 16, 4, 320>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && v2d == 0) rc = launch_variant<3, 16, 0>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && v2d == 161) rc = launch_2d<3, 16, 1>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && v2d == 162) rc = launch_2d<3, 16, 2>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && v2d == 163) rc = launch_2d<3, 16, 3>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && v2d == 17) rc = launch_2s<3>(grid, stream, base, n_rows, d, packed, group_max, gs);
    else if (nq_pad == 256 && S == 3 && v2d == 32) rc = launch_2d<3, 32>(grid, stream, base, n_rows, d, packed, group_max, gs);
    }
    // MSE_SCAN_ABL=32: the 320-query search kernel (64 rows per maximum) WITHOUT its stores of group maxima -- what the dense array
    // of maxima costs the scan (profiles/sparse_maxima_ab.txt); the array keeps whatever an earlier, unablated step left in it
    if (!mask && group_rows == 64 && nq_pad == 320 && getenv("MSE_SCAN_ABL") && atoi(getenv("MSE_SCAN_ABL")) == 32)
        rc = launch_2d<2, 16, 6, 320, 64>(grid, stream, base, n_rows, d, packed, group_max, gs);
    // MSE_SCAN_ABL=33: the same kernel with the cycle stamps of PROF = 1 (mse_dev_scan_prof); its results are the product kernel's
    if (!mask && group_rows == 64 && nq_pad == 320 && getenv("MSE_SCAN_ABL") && atoi(getenv("MSE_SCAN_ABL")) == 33) {
        switch (dev_scan_mid()) {
            case 0: rc = launch_2d<2, 16, 1, 320, 64, 0>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 1: rc = launch_2d<2, 16, 1, 320, 64, 1>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 2: rc = launch_2d<2, 16, 1, 320, 64, 2>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 3: rc = launch_2d<2, 16, 1, 320, 64, 3>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            default: rc = launch_2d<2, 16, 1, 320, 64, 4>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
        }
    }
    // MSE_SCAN_MID alone: the unstamped search kernel on another schedule than the product's (an A/B within one library)
    else if (!mask && group_rows == 64 && nq_pad == 320 && rc == -2 && dev_scan_mid() != MID_320) {
        switch (dev_scan_mid()) {
            case 0: rc = launch_2d<2, 16, 0, 320, 64, 0>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 1: rc = launch_2d<2, 16, 0, 320, 64, 1>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 2: rc = launch_2d<2, 16, 0, 320, 64, 2>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            case 3: rc = launch_2d<2, 16, 0, 320, 64, 3>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
            default: rc = launch_2d<2, 16, 0, 320, 64, 4>(grid, stream, base, n_rows, d, packed, group_max, gs); break;
        }
    }
    if (rc != -2) {
        if (rc) return rc;
        if (ev_end) MSE_HIP_TRY(hipEventRecord(ev_end, stream));
        return 0;
    }
#endif
    // the product configurations below, each unmasked or masked (filtered search: the bitmap as two trailing kernel arguments)
    auto run = [&](auto launch) { return mask ? launch(mask, mask_words) : launch(); };
    if (nq_pad == 320) {
        // 2-D wave split, 64 rows x 160 queries per wave (4 x 10 tiles = 160 accumulator registers; 384 queries per pass spill and
        // run 2.6x slower), two-stage row ring: 2 x 40 KiB of query tiles + 4 x 2 x 8 KiB = 144 KiB (147 456 B) of LDS.
        // Code object (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): unmasked 255 VGPRs, masked 256; both 0
        // spilled, 0 scratch, 2 waves per SIMD.  The 1-D <2,20> kernel this replaced is kept in the developer library (MSE_SCAN_2D=0).
        // group_rows = 64 (the search passes): one maximum per wave's 64 rows instead of two per 32 -- half the array of group maxima,
        // half the 64-byte partial stores, half of what the tournament's first level reads back.  Code object of that form (with the
        // short turn-over of the kernel's header comment): 248 VGPRs unmasked, 250 masked (the mask is applied by selection in the
        // epilogue), 0 spilled, 0 scratch, 2 waves per SIMD -- the same figures with the mid-block schedule (MID_320), which these
        // 64-row forms carry.  The 32-row forms stay on the schedule before it (255 / 256 VGPRs; with MID the masked one spills four).
        // The tile-subset form of that kernel (launch_scan_mfma_tiles, the sparse maxima of api.hip mfma_pass): scan_mfma2d_kernel<2, 16,
        // 0, 320, 64, ScanSparse>: VGPRs: 250, ScratchSize [bytes/lane]: 0, Occupancy [waves/SIMD]: 2, SGPRs Spill: 0, VGPRs Spill: 0.
        if (group_rows == 64) rc = run([&](auto... m) { return launch_2d<2, 16, 0, 320, 64, MID_320>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
        else rc = run([&](auto... m) { return launch_2d<2, 16, 0, 320>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
    } else if (nq_pad == 192) {
        // 12 column tiles on the one-dimensional wave split (32 rows x 192 queries per wave, 96 accumulators): the point between
        // the HBM-bound 128-query pass and the power-bound 256-query pass (profiles/r04_scan_variants.txt)
        rc = run([&](auto... m) { return launch_variant<3, 12, 0>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
    } else if (nq_pad == 128) {
        if (S == 3) rc = run([&](auto... m) { return launch_variant<3, 8, 0>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
        else if (S == 2) rc = run([&](auto... m) { return launch_variant<2, 8, 0>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
        else rc = run([&](auto... m) { return launch_variant<1, 8, 0>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
    } else {
        if (S == 3) rc = run([&](auto... m) { return launch_2d<3, 16>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
        else if (S == 2) rc = run([&](auto... m) { return launch_variant<2, 16, 0>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
        else rc = run([&](auto... m) { return launch_variant<1, 16, 0>(grid, stream, base, n_rows, d, packed, group_max, gs, m...); });
    }
    if (rc) return rc;
    if (ev_end) MSE_HIP_TRY(hipEventRecord(ev_end, stream));
    return 0;
}

int launch_scan_mfma_tiles(const uint16_t* base, size_t n_rows, int d, const uint16_t* queries_dev, int nq_rows, bool pack, void* packed_scratch,
                           const ScanSparse& sp, float* group_max, int n_cu, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end) {
    if (n_rows == 0) return 0;
    if (d % 64 != 0 || d <= 0 || d > D_MAX || (d / KB) % 2 != 0) return fail("scan_mfma_tiles: the 320-query pass needs an even number of K blocks");
    if (sp.tau ? !(sp.counts && sp.ids && sp.keys && sp.cap) : !group_max) return fail("scan_mfma_tiles: no place for the maxima");
    constexpr int BN = 320;
    uint4* packed = reinterpret_cast<uint4*>(packed_scratch);
    if (pack) hipLaunchKernelGGL(pack_queries_kernel, dim3(64, 1), dim3(256), 0, stream, queries_dev, d, BN, nq_rows, packed);
    if (ev_begin) MSE_HIP_TRY(hipEventRecord(ev_begin, stream));
    if (sp.n_tiles) {
        // Code object of this form (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 250 VGPRs, 0 spilled,
        // 0 scratch, 2 waves per SIMD (with the wave index in a vector register and the list offsets hoisted out of the tile loop it
        // spilled 2 to 46 registers: see the kernel's epilogue)
        auto kernel = scan_mfma2d_kernel<2, 16, 0, BN, 64, MID_320, ScanSparse>;
#ifdef MSE_DEV_KERNELS
        {   // MSE_SCAN_ABL=33: cycle stamps; MSE_SCAN_MID: another schedule
            const bool prof = getenv("MSE_SCAN_ABL") && atoi(getenv("MSE_SCAN_ABL")) == 33;
            switch (dev_scan_mid()) {
                case 0: kernel = prof ? scan_mfma2d_kernel<2, 16, 1, BN, 64, 0, ScanSparse> : scan_mfma2d_kernel<2, 16, 0, BN, 64, 0, ScanSparse>; break;
                case 1: kernel = prof ? scan_mfma2d_kernel<2, 16, 1, BN, 64, 1, ScanSparse> : scan_mfma2d_kernel<2, 16, 0, BN, 64, 1, ScanSparse>; break;
                case 2: kernel = prof ? scan_mfma2d_kernel<2, 16, 1, BN, 64, 2, ScanSparse> : scan_mfma2d_kernel<2, 16, 0, BN, 64, 2, ScanSparse>; break;
                case 3: kernel = prof ? scan_mfma2d_kernel<2, 16, 1, BN, 64, 3, ScanSparse> : scan_mfma2d_kernel<2, 16, 0, BN, 64, 3, ScanSparse>; break;
                default: kernel = prof ? scan_mfma2d_kernel<2, 16, 1, BN, 64, 4, ScanSparse> : scan_mfma2d_kernel<2, 16, 0, BN, 64, 4, ScanSparse>; break;
            }
        }
#endif
        const size_t lds = 2 * (size_t)(BN * 128) + (size_t)4 * 2 * 8192 + TAU_SLOTS * sizeof(float);   // 144 KiB + the thresholds' 1.5 KiB
        const size_t n_tiles = (n_rows + TILE_ROWS - 1) / TILE_ROWS;
        const size_t grid = std::min<size_t>((size_t)n_cu, sp.n_tiles);
        MSE_DYN_LDS(kernel, lds);
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid, 1), dim3(W * 64), lds, stream, base, n_rows, d, (const uint4*)packed, group_max, BN, n_tiles,
                           0u, 0u, sp);
        MSE_HIP_TRY(hipGetLastError());
    }
    if (ev_end) MSE_HIP_TRY(hipEventRecord(ev_end, stream));
    return 0;
}

}  // namespace mse

#ifdef MSE_DEV_KERNELS
// developer library only (not in include/mse.h): read and clear the counters of the profiled 2-D scan (MSE_SCAN_2D=161, MSE_SCAN_ABL=33)
extern "C" __attribute__((visibility("default"))) int mse_dev_scan_prof(unsigned long long out[7]) {
    unsigned long long z[7] = {0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mse::g_scan_prof), sizeof(z)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(mse::g_scan_prof), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif
