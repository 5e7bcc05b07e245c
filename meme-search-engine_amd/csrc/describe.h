// Launchers of describe.hip for describe_api.hip.  Every pointer is a device pointer; every launch goes to `st` and does not wait.
#pragma once
#include "runtime.h"

namespace mse {

constexpr int SEL_MAX_RANKS = 512;                 // ranks per select
constexpr int SEL_BINS12 = 2048, SEL_BINS3 = 1024; // 11 / 11 / 10 bits
constexpr uint32_t SEL_NO_SLOT = 0xFFFFu;

// fixed-size scratch of one select, n-independent (u32 words, in this order)
struct SelectScratch {
    uint32_t* cnt1;     // [2048]              top-digit counts
    uint32_t* cnt2;     // [512][2048]         second-digit counts of the selected top digits
    uint32_t* cnt3;     // [512][1024]         last-digit counts of the selected 22-bit prefixes
    uint32_t* n_nan;    // [1]
    uint32_t* rem;      // [512]               in: the ranks; after each resolve: the rank within the bucket
    uint32_t* prefix;   // [512]               the digits resolved so far; after the third resolve: the keys
    uint32_t* slot;     // [512]               counter row of each rank's prefix in the next pass
    uint32_t* sorted;   // [512]               the distinct prefixes, ascending (slot -> prefix)
    uint32_t* n_slots;  // [1]
    uint16_t* slot1;    // [2048]              top digit -> slot, SEL_NO_SLOT when not selected
};
constexpr size_t SEL_COUNTER_WORDS = SEL_BINS12 + (size_t)SEL_MAX_RANKS * SEL_BINS12 + (size_t)SEL_MAX_RANKS * SEL_BINS3 + 1;
constexpr size_t SEL_SCRATCH_WORDS = SEL_COUNTER_WORDS + 4 * SEL_MAX_RANKS + 1 + SEL_BINS12 / 2 + 16;
SelectScratch select_scratch_at(uint32_t* base);   // the counters (cnt1 .. n_nan) come first and contiguous: one memset clears them

// scores[i][c], i < n, of the base rows ids[i] (ids null: first + i); rows f16 [.][d], d == the model's d_emb
void launch_score_mlp(const uint16_t* rows, int d, const uint32_t* ids, size_t first, size_t n, const float* up, const float* bias,
                      const float* down, int d_hidden, int out_ch, float* scores, hipStream_t st);
// pass 1 .. 3 of the select over keys data[i * stride], i < n (as_f32: f32 through the order-preserving transform, else plain u32)
void launch_select_count(int pass, const uint32_t* data, size_t stride, size_t n, int as_f32, const SelectScratch& sc, hipStream_t st);
// after pass `level`: descend each of the n_ranks ranks into its bucket, then number the distinct prefixes for the next pass
void launch_select_resolve(int level, const SelectScratch& sc, int n_ranks, hipStream_t st);
// desc[row][j] = bucket(cdfs[j], value_j) for row = ids[i] (ids null: first + i), i < n; value_j = scores[i][j] for j < n_ch, (float)ts[i]
// for the last channel when ts is not null; n_desc = n_ch + (ts ? 1 : 0)
void launch_describe(const float* cdfs, int cdf_len, const float* scores, int n_ch, const uint32_t* ts, const uint32_t* ids, size_t first,
                     size_t n, uint8_t* desc, int n_desc, hipStream_t st);

}  // namespace mse
