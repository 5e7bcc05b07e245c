// The near-duplicate self-join (include/mse.h mse_join_self): every unordered pair of base rows whose reference-order score
// reaches a threshold, and the keep-first rule over the resulting pair list.
//
// Schedule.  The Gram matrix of the base is cut into JOIN_TILE x JOIN_TILE tiles; only tiles of the lower triangle that meet the `window`
// band exist.  A STRIP is a run of hi-tile rows; its tiles are numbered t = (hi tile - first hi tile) * span + x, lo tile = hi tile - x
// (x = 0: the diagonal tile).  A workgroup owns one tile, counts the pairs it nominates, gives each a RANK inside the tile that depends on
// nothing but the tile's data (thread order, then accumulator order), and stores them at tile base + rank:
//   first launch of a strip   the base is reserved with one atomic per tile, so the buffer holds whole tiles in arrival order; if the
//                             strip's nominations fit, they are complete and their order does not matter (the list is sorted at the end);
//   a strip that did not fit  the tile counts of the first launch are scanned in tile order, and the strip is launched again once per
//                             buffer-sized window of that numbering: a tile outside the window leaves at once, a tile inside stores the
//                             ranks that fall into it.  Every nomination is stored in exactly one window, whatever the buffer's size.
// MFMA tiles nominate by `accumulator >= threshold - bound` (mfma_pair_bound: the certificate of DESIGN.md 3.2); exact tiles nominate by the
// exact score itself.  Either way a lane quad re-scores each nominated pair in reference order (exact_dot.h) and only pairs at or above the
// threshold are kept, so the kept set is the same in every mode.
//
// The cross join (mse_join_cross) runs the same tiles over a rectangle: the hi role is a row of a second, incoming base, the lo
// role a row of the resident one (kernels.h JoinStrip).  the CROSS = true instances of the tile kernels take both bases, as does the re-score;
// there is no triangle and no window, and `within` speaks for the resident rows only.  Workgroups that are resident together (blockIdx.x
// fastest: the incoming tiles) share a base tile.
#include "common.h"
#include "kernels.h"
#include "exact_dot.h"
#include <algorithm>

namespace mse {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

constexpr int JT = JOIN_TILE;        // rows per tile side
constexpr int KC = 64;               // f16 values of K per LDS stage
constexpr int LROW = KC * 2 + 16;    // bytes of one staged row: 128 of data + 16 of padding (b128 reads of 32 consecutive rows spread over the banks)
constexpr int PANEL = JT * LROW;     // bytes of one operand panel of one stage

struct TileGeom {
    uint32_t th, tl;     // hi and lo tile
    uint32_t t;          // number in the strip
    bool live;
};

template <bool CROSS>
__device__ __forceinline__ TileGeom tile_of_block(const JoinStrip& sp) {
    TileGeom g;
    if (CROSS) {   // hi: the incoming tile, lo: the base tile; the grid is the strip's rectangle
        g.th = sp.x0 + blockIdx.x;
        g.tl = sp.h0 + blockIdx.y;
        g.t = blockIdx.y * sp.span + blockIdx.x;
        g.live = true;
        return g;
    }
    g.th = sp.h0 + blockIdx.y;
    g.t = blockIdx.y * sp.span + blockIdx.x;
    g.live = blockIdx.x <= g.th;
    g.tl = g.live ? g.th - blockIdx.x : 0u;
    if (g.live && sp.window) {   // the closest pair of the two tiles: lowest hi row against highest lo row
        const uint64_t hi_min = (uint64_t)g.th * JT, lo_max = (uint64_t)g.tl * JT + (JT - 1);
        if (hi_min > lo_max && hi_min - lo_max > sp.window) g.live = false;
    }
    return g;
}

// the 128 `within` bits of a tile's rows (null: all ones), masked to the rows below n
__device__ __forceinline__ void tile_bits(const uint32_t* __restrict__ within, size_t within_words, uint32_t tile, uint32_t n, uint32_t (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const size_t w = (size_t)tile * (JT / 32) + i;
        const uint64_t r0 = (uint64_t)w * 32;
        uint32_t v = within ? (w < within_words ? within[w] : 0u) : 0xffffffffu;
        if (r0 >= n) v = 0u;
        else if (r0 + 32 > n) v &= 0xffffffffu >> (32 - (n - r0));
        out[i] = v;
    }
}

__device__ __forceinline__ bool bit_of(const uint32_t (&b)[4], int r) {
    const uint32_t w = r < 32 ? b[0] : r < 64 ? b[1] : r < 96 ? b[2] : b[3];
    return (w >> (r & 31)) & 1u;
}

// exclusive prefix of v over the 256 threads of the block (thread order) and the block's total
__device__ __forceinline__ uint32_t block_rank(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t s = wave_sums[w];
        if (w < wave) base += s;
        all += s;
    }
    *total = all;
    return base + inc - v;
}

// Where this tile's nominations go.  Returns false when the tile stores nothing in this launch; otherwise slot = *base + rank is stored iff
// lo_slot <= slot < hi_slot (as cand[slot - lo_slot]).
__device__ __forceinline__ bool tile_placement(const JoinStrip& sp, uint32_t t, uint32_t total, uint32_t* lds_base, unsigned long long* base,
                                               unsigned long long* lo_slot, unsigned long long* hi_slot) {
    if (sp.tile_base) {   // a window of the scanned numbering
        *base = sp.tile_base[t];
        *lo_slot = sp.win_lo;
        *hi_slot = sp.win_lo + sp.cap;
        return true;
    }
    if (threadIdx.x == 0) {
        sp.tile_count[t] = total;
        unsigned long long b = 0;
        if (total) b = atomicAdd(sp.cursor, (unsigned long long)total);
        lds_base[0] = (uint32_t)b; lds_base[1] = (uint32_t)(b >> 32);
    }
    __syncthreads();
    *base = (unsigned long long)lds_base[0] | ((unsigned long long)lds_base[1] << 32);
    *lo_slot = 0;
    *hi_slot = sp.cap;
    return total != 0 && *base + total <= sp.cap;   // whole tiles only: a strip that overflows is run again in windows
}

// ---- the matrix-core tile ---------------------------------------------------------------------------------------------------------------
// 256 threads = four waves in a 2 x 2 arrangement, each 64 x 64 of the tile as 2 x 2 blocks of v_mfma_f32_32x32x16_f16 (64 accumulator
// registers).  Both operand panels (128 rows x 64 f16 of K) go through LDS in two stages: the global loads of stage s + 1 are issued before
// the products of stage s and written to the other buffer after them, one barrier per stage.  Rows at or past n are read as row n - 1 and
// excluded in the epilogue.
// CROSS: hi rows come from `incoming` (n_inc rows), lo rows from `base`; every row below n_inc counts on the hi side, `within` on the lo side.
template <bool CROSS>
__global__ __launch_bounds__(256, 2) void join_tile_mfma_kernel(const uint16_t* __restrict__ base, uint32_t n, const uint16_t* __restrict__ incoming,
                                                                uint32_t n_inc, int d, JoinStrip sp, double thr_lo) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint32_t wave_sums[4];
    __shared__ uint32_t lds_base[2];
    const uint16_t* __restrict__ rows_hi = CROSS ? incoming : base;
    const uint32_t n_hi = CROSS ? n_inc : n;
    const TileGeom g = tile_of_block<CROSS>(sp);
    if (!g.live) return;
    if (sp.tile_base) {   // a window launch: tiles without a slot in the window leave before any work
        const unsigned long long b = sp.tile_base[g.t], c = sp.tile_count[g.t];
        if (c == 0 || b + c <= sp.win_lo || b >= sp.win_lo + sp.cap) return;
    }
    uint32_t hb[4], lb[4];
    tile_bits(CROSS ? nullptr : sp.within, sp.within_words, g.th, n_hi, hb);
    tile_bits(sp.within, sp.within_words, g.tl, n, lb);
    if (!(hb[0] | hb[1] | hb[2] | hb[3]) || !(lb[0] | lb[1] | lb[2] | lb[3])) {   // a tile whose rows are all excluded
        if (!sp.tile_base && threadIdx.x == 0) sp.tile_count[g.t] = 0;
        return;
    }
    if (!sp.tile_base && threadIdx.x == 0) atomicAdd(sp.tiles_run, 1ull);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // staging: a panel stage is 128 rows x 8 pieces of 16 bytes; thread tid moves pieces tid, tid + 256, tid + 512, tid + 768
    const uint16_t* src[2][4];
    int dst[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int p = tid + 256 * i, row = p >> 3, piece = p & 7;
        const uint64_t rh = (uint64_t)g.th * JT + row, rl = (uint64_t)g.tl * JT + row;
        src[0][i] = rows_hi + (size_t)(rh < n_hi ? rh : n_hi - 1) * d + piece * 8;
        src[1][i] = base + (size_t)(rl < n ? rl : n - 1) * d + piece * 8;
        dst[i] = row * LROW + piece * 16;
    }
    float16v acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[a][b][v] = 0.0f;

    uint4 ra[4], rb[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { ra[i] = *reinterpret_cast<const uint4*>(src[0][i]); rb[i] = *reinterpret_cast<const uint4*>(src[1][i]); }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        *reinterpret_cast<uint4*>(lds + dst[i]) = ra[i];
        *reinterpret_cast<uint4*>(lds + PANEL + dst[i]) = rb[i];
    }
    __syncthreads();
    const int stages = d / KC;
    // this lane's fragment address inside a panel: row (lane & 31) of the wave's 32-row block, K piece lane >> 5
    const int frag = (lane & 31) * LROW + (lane >> 5) * 16;
    for (int s = 0; s < stages; s++) {
        const unsigned char* cur = lds + (s & 1) * 2 * PANEL;
        unsigned char* nxt = lds + ((s + 1) & 1) * 2 * PANEL;
        // the stage fetched ahead is clamped to the last one instead of being made conditional (as exact_dot.h does): the last stage's
        // copy goes to the buffer nobody reads any more
        const size_t ahead = (size_t)(s + 1 < stages ? s + 1 : s) * KC;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            ra[i] = *reinterpret_cast<const uint4*>(src[0][i] + ahead);
            rb[i] = *reinterpret_cast<const uint4*>(src[1][i] + ahead);
        }
#pragma unroll
        for (int ks = 0; ks < KC / 16; ks++) {
            half8 fa[2], fb[2];
#pragma unroll
            for (int a = 0; a < 2; a++) fa[a] = *reinterpret_cast<const half8*>(cur + (wr * 64 + a * 32) * LROW + frag + ks * 32);
#pragma unroll
            for (int b = 0; b < 2; b++) fb[b] = *reinterpret_cast<const half8*>(cur + PANEL + (wc * 64 + b * 32) * LROW + frag + ks * 32);
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *reinterpret_cast<uint4*>(nxt + dst[i]) = ra[i];
            *reinterpret_cast<uint4*>(nxt + PANEL + dst[i]) = rb[i];
        }
        __syncthreads();
    }

    // epilogue: accumulator v of block (a, b) is row (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of the A block, column lane & 31 of the B block
    const uint64_t hi0 = (uint64_t)g.th * JT, lo0 = (uint64_t)g.tl * JT;
    uint64_t hit = 0;   // bit a * 32 + b * 16 + v
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int cl = wc * 64 + b * 32 + (lane & 31);
            const uint64_t lo = lo0 + cl;
            const bool col_ok = bit_of(lb, cl);
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int rl = wr * 64 + a * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
                const uint64_t hi = hi0 + rl;
                bool ok = col_ok && (CROSS || lo < hi) && bit_of(hb, rl) && (CROSS || sp.window == 0 || hi - lo <= sp.window);
                ok = ok && (double)acc[a][b][v] * 4294967296.0 >= thr_lo;
                hit |= (uint64_t)ok << (a * 32 + b * 16 + v);
            }
        }
    uint32_t total;
    const uint32_t rank0 = block_rank((uint32_t)__popcll(hit), wave_sums, &total);
    unsigned long long tbase, lo_slot, hi_slot;
    if (!tile_placement(sp, g.t, total, lds_base, &tbase, &lo_slot, &hi_slot)) return;
    unsigned long long slot = tbase + rank0;
    uint64_t m = hit;
    while (m) {
        const int bit = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int a = bit >> 5, b = (bit >> 4) & 1, v = bit & 15;
        if (slot >= lo_slot && slot < hi_slot) {
            const uint32_t hi = (uint32_t)(hi0 + wr * 64 + a * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5));
            const uint32_t lo = (uint32_t)(lo0 + wc * 64 + b * 32 + (lane & 31));
            sp.cand[slot - lo_slot] = make_uint2(lo, hi);
        }
        slot++;
    }
}

// ---- the exact tile: every pair of the tile on the vector ALU in reference order ----------------------------------------------------
// 64 lane quads; quad q scores pairs p = q, q + 64, ...: hi row p / 128, lo row p % 128 of the tile.  STORE = false counts the quad's hits,
// STORE = true scores the tile again and stores them -- only tiles with a hit are scored twice.
template <bool STORE, bool CROSS>
__device__ __forceinline__ uint32_t exact_tile_pass(const uint16_t* __restrict__ rows_hi, const uint16_t* __restrict__ base, int d, const JoinStrip& sp, const TileGeom& g,
                                                    const uint32_t (&hb)[4], const uint32_t (&lb)[4], int64_t threshold,
                                                    unsigned long long slot, unsigned long long lo_slot, unsigned long long hi_slot) {
    const int q = threadIdx.x >> 2;
    const uint64_t hi0 = (uint64_t)g.th * JT, lo0 = (uint64_t)g.tl * JT;
    uint32_t hits = 0;
    for (int p = q; p < JT * JT; p += 64) {
        const int rl = p / JT, cl = p % JT;
        const uint64_t hi = hi0 + rl, lo = lo0 + cl;
        if (!((CROSS || lo < hi) && bit_of(hb, rl) && bit_of(lb, cl) && (CROSS || sp.window == 0 || hi - lo <= sp.window))) continue;   // the same for the quad's four lanes
        const float f = quad_fast_dot_f32(rows_hi + (size_t)hi * d, base + (size_t)lo * d, d);
        if (scale_dot_result(f) < threshold) continue;
        if (STORE && (threadIdx.x & 3) == 0 && slot + hits >= lo_slot && slot + hits < hi_slot)
            sp.cand[slot + hits - lo_slot] = make_uint2((uint32_t)lo, (uint32_t)hi);
        hits++;
    }
    return hits;
}

template <bool CROSS>
__global__ __launch_bounds__(256) void join_tile_exact_kernel(const uint16_t* __restrict__ base, uint32_t n, const uint16_t* __restrict__ incoming, uint32_t n_inc,
                                                              int d, JoinStrip sp, int64_t threshold) {
    __shared__ uint32_t wave_sums[4];
    __shared__ uint32_t lds_base[2];
    const uint16_t* __restrict__ rows_hi = CROSS ? incoming : base;
    const uint32_t n_hi = CROSS ? n_inc : n;
    const TileGeom g = tile_of_block<CROSS>(sp);
    if (!g.live) return;
    if (sp.tile_base) {
        const unsigned long long b = sp.tile_base[g.t], c = sp.tile_count[g.t];
        if (c == 0 || b + c <= sp.win_lo || b >= sp.win_lo + sp.cap) return;
    }
    uint32_t hb[4], lb[4];
    tile_bits(CROSS ? nullptr : sp.within, sp.within_words, g.th, n_hi, hb);
    tile_bits(sp.within, sp.within_words, g.tl, n, lb);
    if (!(hb[0] | hb[1] | hb[2] | hb[3]) || !(lb[0] | lb[1] | lb[2] | lb[3])) {
        if (!sp.tile_base && threadIdx.x == 0) sp.tile_count[g.t] = 0;
        return;
    }
    if (!sp.tile_base && threadIdx.x == 0) atomicAdd(sp.tiles_run, 1ull);
    const uint32_t hits = exact_tile_pass<false, CROSS>(rows_hi, base, d, sp, g, hb, lb, threshold, 0, 0, 0);
    uint32_t total;
    // one count per quad: its first lane speaks for it
    const uint32_t rank0 = block_rank((threadIdx.x & 3) == 0 ? hits : 0u, wave_sums, &total);
    unsigned long long tbase, lo_slot, hi_slot;
    if (!tile_placement(sp, g.t, total, lds_base, &tbase, &lo_slot, &hi_slot)) return;
    const unsigned long long quad_slot = tbase + __shfl(rank0, (threadIdx.x & 63) & ~3);
    (void)exact_tile_pass<true, CROSS>(rows_hi, base, d, sp, g, hb, lb, threshold, quad_slot, lo_slot, hi_slot);
}

// exclusive prefix of the strip's tile counts, in tile order (one workgroup; each thread walks a contiguous run)
__global__ __launch_bounds__(256) void join_scan_tiles_kernel(const uint32_t* __restrict__ counts, size_t n_tiles, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[256];
    const size_t per = (n_tiles + 255) / 256;
    const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < n_tiles ? lo + per : n_tiles;
    unsigned long long s = 0;
    for (size_t b = lo; b < hi; b++) s += counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 256; t++) { const unsigned long long v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (size_t b = lo; b < hi; b++) { out[b] = run; run += counts[b]; }
}

// ---- the re-score: a lane quad per nominated pair ----------------------------------------------------------------------------------------
// counters[0] += pairs at or above the threshold; while the running count stays within store_cap the pair is appended to conf (in arrival
// order: the list is put into canonical order at the end) and counted into row_count[hi]
// (rows_hi: the base again, or the cross join's incoming rows)
__global__ __launch_bounds__(256) void join_rescore_kernel(const uint16_t* __restrict__ base, const uint16_t* __restrict__ rows_hi, int d, const uint2* __restrict__ cand, size_t m,
                                                           int64_t threshold, unsigned long long* __restrict__ kept, JoinPair* __restrict__ conf,
                                                           unsigned long long store_cap, uint32_t* __restrict__ row_count) {
    const size_t quads = ((size_t)gridDim.x * blockDim.x) >> 2;
    const size_t steps = (m + quads - 1) / quads;   // every quad runs the same number of steps: whole quads stay together
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    for (size_t s = 0; s < steps; s++, i += quads) {
        if (i >= m) continue;   // (the quad's four lanes share i)
        const uint2 p = cand[i];
        const int64_t sc = scale_dot_result(quad_fast_dot_f32(rows_hi + (size_t)p.y * d, base + (size_t)p.x * d, d));
        if (sc >= threshold && (threadIdx.x & 3) == 0) {
            const unsigned long long at = atomicAdd(kept, 1ull);
            if (at < store_cap) {
                conf[at] = JoinPair{p.x, p.y, sc};
                atomicAdd(&row_count[p.y], 1u);
            }
        }
    }
}

// ---- the list in canonical order: a CSR over hi --------------------------------------------------------------------------------------------
// offsets[r] = pairs of the rows below r, r = 0 .. n (one workgroup, as join_scan_tiles_kernel)
__global__ __launch_bounds__(256) void join_offsets_kernel(const uint32_t* __restrict__ row_count, size_t n, unsigned long long* __restrict__ offsets) {
    __shared__ unsigned long long part[256];
    const size_t per = (n + 255) / 256;
    const size_t lo = (size_t)threadIdx.x * per < n ? (size_t)threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    unsigned long long s = 0;
    for (size_t b = lo; b < hi; b++) s += row_count[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 256; t++) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        offsets[n] = run;
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (size_t b = lo; b < hi; b++) { offsets[b] = run; run += row_count[b]; }
}

// pair i goes to some free position of its row's segment: row_count counts down
__global__ void join_fill_kernel(const JoinPair* __restrict__ conf, size_t count, const unsigned long long* __restrict__ offsets,
                                 uint32_t* __restrict__ row_count, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, int64_t* __restrict__ scores) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const JoinPair p = conf[i];
    const size_t at = offsets[p.hi] + (atomicSub(&row_count[p.hi], 1u) - 1u);
    lo[at] = p.lo; hi[at] = p.hi; scores[at] = p.score;
}

__device__ __forceinline__ void sift_down(uint32_t* lo, int64_t* sc, size_t root, size_t end) {
    for (;;) {
        size_t child = 2 * root + 1;
        if (child >= end) return;
        if (child + 1 < end && lo[child + 1] > lo[child]) child++;
        if (lo[root] >= lo[child]) return;
        const uint32_t tl = lo[root]; lo[root] = lo[child]; lo[child] = tl;
        const int64_t ts = sc[root]; sc[root] = sc[child]; sc[child] = ts;
        root = child;
    }
}

// each row's segment by ascending lo (a row's lo values are distinct, so the order is unique): one thread per row, heap sort in place
__global__ void join_sort_rows_kernel(const unsigned long long* __restrict__ offsets, size_t n, uint32_t* __restrict__ lo, int64_t* __restrict__ scores) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const size_t b = offsets[r], m = offsets[r + 1] - b;
    if (m < 2) return;
    uint32_t* l = lo + b;
    int64_t* s = scores + b;
    for (size_t i = m / 2; i-- > 0;) sift_down(l, s, i, m);
    for (size_t end = m - 1; end > 0; end--) {
        const uint32_t tl = l[0]; l[0] = l[end]; l[end] = tl;
        const int64_t ts = s[0]; s[0] = s[end]; s[end] = ts;
        sift_down(l, s, 0, end);
    }
}

// ---- keep-first over the CSR ---------------------------------------------------------------------------------------------------------------
// state: 0 undecided, 1 kept, 2 dropped.  A round reads `in` and writes `out` (all rows), so a round's outcome does not depend on the order
// its threads run in: dropped as soon as one earlier neighbour is kept, kept once all are dropped.  *undecided += rows still open
__global__ void join_round_kernel(const unsigned long long* __restrict__ offsets, const uint32_t* __restrict__ lo, size_t n,
                                  const uint8_t* __restrict__ in, uint8_t* __restrict__ out, unsigned long long* __restrict__ undecided) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    uint8_t st = in[r];
    if (st == 0) {
        bool open = false, drop = false;
        for (unsigned long long e = offsets[r]; e < offsets[r + 1] && !drop; e++) {
            const uint8_t ns = in[lo[e]];
            drop = ns == 1;
            open = open || ns == 0;
        }
        st = drop ? 2 : open ? 0 : 1;
        if (st == 0) atomicAdd(undecided, 1ull);
    }
    out[r] = st;
}

// rep[r] = r for a kept row, its lowest kept earlier neighbour for a dropped one; has_member[rep] = 1 for every dropped row's representative;
// dup: the dropped rows as bitmap words (whole 256-row tiles, zero past n)
__global__ __launch_bounds__(256) void join_rep_kernel(const unsigned long long* __restrict__ offsets, const uint32_t* __restrict__ lo, size_t n,
                                                       const uint8_t* __restrict__ state, uint32_t* __restrict__ rep, uint8_t* __restrict__ has_member,
                                                       uint32_t* __restrict__ dup) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool dropped = false;
    if (r < n) {
        uint32_t v = (uint32_t)r;
        if (state[r] == 2) {
            dropped = true;
            for (unsigned long long e = offsets[r]; e < offsets[r + 1]; e++)
                if (state[lo[e]] == 1) { v = lo[e]; break; }   // ascending: the first kept one is the lowest
            has_member[v] = 1;
        }
        rep[r] = v;
    }
    const unsigned long long m = __ballot(dropped);
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<uint2*>(dup + (r >> 6) * 2) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
}

__global__ void join_labels_kernel(const uint32_t* __restrict__ rep, const uint8_t* __restrict__ has_member, size_t n, uint32_t* __restrict__ labels) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t v = rep[r];
    labels[r] = (v != (uint32_t)r || has_member[r]) ? v : ID_NONE;
}

// ---- admission: keep-first continued from the resident rows into the incoming ones --------------------------------------------------
// The resident rows come first in the walk and are all kept, so an incoming row with a cross pair is dropped before any round runs; the
// rounds of join_round_kernel over the list AMONG the incoming rows then start from that state.  decide: there is no such list, the rest
// is kept at once.
__global__ void join_admit_init_kernel(const unsigned long long* __restrict__ cross_offsets, size_t m, bool decide, uint8_t* __restrict__ state,
                                       unsigned long long* __restrict__ undecided) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint8_t st = cross_offsets[j + 1] > cross_offsets[j] ? 2 : decide ? 1 : 0;
    state[j] = st;
    if (st == 0) atomicAdd(undecided, 1ull);
}

__global__ __launch_bounds__(256) void join_admit_finish_kernel(const unsigned long long* __restrict__ cross_offsets, const uint32_t* __restrict__ cross_lo,
                                                                const unsigned long long* __restrict__ among_offsets,
                                                                const uint32_t* __restrict__ among_lo, size_t m, const uint8_t* __restrict__ state,
                                                                uint32_t* __restrict__ rep_base, uint32_t* __restrict__ rep_incoming,
                                                                uint32_t* __restrict__ kept_words) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    if (j < m) {
        const unsigned long long c0 = cross_offsets[j];
        const bool by_base = cross_offsets[j + 1] > c0;
        rep_base[j] = by_base ? cross_lo[c0] : ID_NONE;   // ascending: the first one is the lowest
        kept = state[j] == 1;
        uint32_t v = kept ? (uint32_t)j : ID_NONE;
        if (!kept && !by_base && among_offsets)
            for (unsigned long long e = among_offsets[j]; e < among_offsets[j + 1]; e++)
                if (state[among_lo[e]] == 1) { v = among_lo[e]; break; }
        rep_incoming[j] = v;
    }
    const unsigned long long w = __ballot(kept);
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<uint2*>(kept_words + (j >> 6) * 2) = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
}

// ---- the selected rows of a base, packed: 16-byte pieces, consecutive threads on consecutive pieces of a row -------------------------
__global__ __launch_bounds__(256) void join_select_rows_kernel(const uint4* __restrict__ in, size_t row_u4, const uint32_t* __restrict__ ids, size_t count,
                                                               uint4* __restrict__ out) {
    const size_t total = count * row_u4, step = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const size_t j = t / row_u4, c = t - j * row_u4;
        out[t] = in[(size_t)ids[j] * row_u4 + c];
    }
}

inline unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

size_t join_tile_lds_bytes() { return 4 * PANEL; }

template <bool CROSS>
static int launch_join_tiles_of(bool exact, const uint16_t* base, size_t n, const uint16_t* incoming, size_t m, int d, const JoinStrip& sp,
                                int64_t threshold, double thr_lo, hipStream_t stream) {
    const dim3 grid(sp.span, sp.n_hi), block(256);
    if (exact) {
        hipLaunchKernelGGL(join_tile_exact_kernel<CROSS>, grid, block, 0, stream, base, (uint32_t)n, incoming, (uint32_t)m, d, sp, threshold);
    } else {
        if (d % KC) return fail("join: the matrix-core tile needs a width that is a multiple of 64");
        MSE_DYN_LDS(join_tile_mfma_kernel<CROSS>, join_tile_lds_bytes());
        hipLaunchKernelGGL(join_tile_mfma_kernel<CROSS>, grid, block, join_tile_lds_bytes(), stream, base, (uint32_t)n, incoming, (uint32_t)m, d, sp, thr_lo);
    }
    return 0;
}

int launch_join_tiles(bool exact, const uint16_t* base, size_t n, const uint16_t* incoming, size_t m, int d, const JoinStrip& sp, int64_t threshold,
                      double thr_lo, hipStream_t stream) {
    if (sp.n_hi == 0 || sp.span == 0) return 0;
    if (sp.n_hi > 65535) return fail("join: more than 65535 tile rows in a strip");
    if (incoming) {   // every tile of the rectangle must lie inside both bases: the kernels clamp rows, not tiles
        if (n == 0 || m == 0 || (size_t)sp.h0 + sp.n_hi > (n + JT - 1) / JT || (size_t)sp.x0 + sp.span > (m + JT - 1) / JT)
            return fail("join: a strip of the cross join reaches past its bases");
        if (launch_join_tiles_of<true>(exact, base, n, incoming, m, d, sp, threshold, thr_lo, stream)) return -1;
    } else if (launch_join_tiles_of<false>(exact, base, n, nullptr, 0, d, sp, threshold, thr_lo, stream)) return -1;
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_scan_tiles(const uint32_t* counts, size_t n_tiles, unsigned long long* out, hipStream_t stream) {
    if (n_tiles == 0) return 0;
    hipLaunchKernelGGL(join_scan_tiles_kernel, dim3(1), dim3(256), 0, stream, counts, n_tiles, out);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_rescore(const uint16_t* base, const uint16_t* incoming, int d, const uint2* cand, size_t m, int64_t threshold, unsigned long long* kept, JoinPair* conf,
                        unsigned long long store_cap, uint32_t* row_count, int n_cu, hipStream_t stream) {
    if (m == 0) return 0;
    const size_t want = (m + 63) / 64;   // 64 quads per block
    const unsigned blocks = (unsigned)std::min<size_t>(want, (size_t)std::max(n_cu, 1) * 16);
    hipLaunchKernelGGL(join_rescore_kernel, dim3(blocks), dim3(256), 0, stream, base, incoming ? incoming : base, d, cand, m, threshold, kept, conf,
                       store_cap, row_count);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_csr(const JoinPair* conf, size_t count, size_t n, uint32_t* row_count, unsigned long long* offsets, uint32_t* lo, uint32_t* hi,
                    int64_t* scores, hipStream_t stream) {
    hipLaunchKernelGGL(join_offsets_kernel, dim3(1), dim3(256), 0, stream, row_count, n, offsets);
    if (count) {
        hipLaunchKernelGGL(join_fill_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, stream, conf, count, offsets, row_count, lo, hi, scores);
        hipLaunchKernelGGL(join_sort_rows_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, offsets, n, lo, scores);
    }
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_round(const unsigned long long* offsets, const uint32_t* lo, size_t n, const uint8_t* in, uint8_t* out, unsigned long long* undecided,
                      hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(join_round_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, offsets, lo, n, in, out, undecided);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_finish(const unsigned long long* offsets, const uint32_t* lo, size_t n, const uint8_t* state, uint32_t* rep, uint8_t* has_member,
                       uint32_t* dup_words, uint32_t* labels, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(join_rep_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, offsets, lo, n, state, rep, has_member, dup_words);
    hipLaunchKernelGGL(join_labels_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, rep, has_member, n, labels);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_admit_init(const unsigned long long* cross_offsets, size_t m, bool decide, uint8_t* state, unsigned long long* undecided,
                           hipStream_t stream) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(join_admit_init_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, stream, cross_offsets, m, decide, state, undecided);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_admit_finish(const unsigned long long* cross_offsets, const uint32_t* cross_lo, const unsigned long long* among_offsets,
                             const uint32_t* among_lo, size_t m, const uint8_t* state, uint32_t* rep_base, uint32_t* rep_incoming,
                             uint32_t* kept_words, hipStream_t stream) {
    if (m == 0) return 0;
    hipLaunchKernelGGL(join_admit_finish_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, stream, cross_offsets, cross_lo, among_offsets, among_lo, m,
                       state, rep_base, rep_incoming, kept_words);
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_join_select_rows(const void* in, size_t row_bytes, const uint32_t* ids, size_t count, void* out, int n_cu, hipStream_t stream) {
    const size_t total = count * (row_bytes / 16);
    if (total == 0) return 0;
    if (row_bytes % 16 || (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16)
        return fail("select rows: rows must be whole 16-byte pieces at 16-byte aligned addresses");
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)std::max(n_cu, 1) * 32);
    hipLaunchKernelGGL(join_select_rows_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint4*>(in), row_bytes / 16, ids, count,
                       reinterpret_cast<uint4*>(out));
    MSE_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mse
