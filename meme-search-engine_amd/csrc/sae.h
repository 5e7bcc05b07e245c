// Launchers of sae.hip for sae_api.hip.  Every pointer is a device pointer; every launch goes to `st` and does not wait.
#pragma once
#include "runtime.h"

namespace mse {

constexpr int SAE_ROW_TILE = 128, SAE_HID_TILE = 128;   // rows per workgroup; hidden units per step of a workgroup
constexpr int SAE_MAX_TOP_K = 256;
constexpr int SAE_MAX_PARTS = 1024;                     // hidden parts of one call (grid y)
constexpr uint32_t SAE_NONE = 0xFFFFFFFFu;              // an unused feature slot; the count of an invalid row

constexpr int SAE_LIST_SLACK = 256;                     // entries a candidate list may gather beyond that before it is cut

// entries of one (row, part) candidate list: the best top_k + 1, the slack, and what one hidden tile can add
inline size_t sae_list_cap(size_t top_k) { return top_k + 1 + SAE_HID_TILE + SAE_LIST_SLACK; }

// downT[h][e] = down[e][h]
void launch_sae_transpose(const float* down, size_t d_emb, size_t d_hidden, float* downT, hipStream_t st);
// the candidate lists of rows ids[i] (ids null: first + i), i < n: part p of parts walks the hidden tiles p tiles_per_part .. and leaves
// in lists[(i * parts + p) * cap ..] its best pcount[i * parts + p] <= top_k + 1 keys, descending; pflag: a NaN pre-activation was seen.
// lists, pcount and pflag hold whole row tiles: ceil(n / 128) * 128 rows
void launch_sae_encode(const uint16_t* rows, int d, const uint32_t* ids, size_t first, size_t n, const float* up, const float* up_bias,
                       int d_hidden, int top_k, int parts, int tiles_per_part, unsigned long long* lists, uint32_t* pcount, uint32_t* pflag,
                       hipStream_t st);
// counts[i], feats[i][top_k], acts[i][top_k] from the parts' lists; counters (may be null) += 1 per kept feature; *n_invalid += invalid rows
void launch_sae_merge(const unsigned long long* lists, const uint32_t* pcount, const uint32_t* pflag, int parts, int top_k, size_t n,
                      uint32_t* counts, uint32_t* feats, float* acts, unsigned long long* counters, uint32_t* n_invalid, hipStream_t st);
// recon[i][d] (may be null) and sqerr[i] (may be null) of the table rows i < n against the source rows ids[i] / first + i
void launch_sae_reconstruct(const uint32_t* counts, const uint32_t* feats, const float* acts, int top_k, const float* downT, const float* down_bias,
                            int d, const uint16_t* rows, const uint32_t* ids, size_t first, size_t n, float* recon, double* sqerr, hipStream_t st);
// bit ids[i] / first + i of `words` is set where table row i keeps `feature` with activation >= min_activation (words zeroed by the caller)
void launch_sae_feature_bits(const uint32_t* counts, const uint32_t* feats, const float* acts, int top_k, size_t n, const uint32_t* ids, size_t first,
                             uint32_t feature, float min_activation, uint32_t* words, hipStream_t st);

}  // namespace mse
