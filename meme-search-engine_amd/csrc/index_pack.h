// What index_pack.hip (host-in / host-out score model, descriptor buckets) and describe.hip / describe_api.hip (the same over a resident
// index) share: the score model's handle and the Rust-faithful bucket search.
#pragma once
#include "runtime.h"

struct mse_score_model {
    float *up = nullptr, *bias = nullptr, *down = nullptr;  // device
    size_t d_emb = 0, d_hidden = 0, out_ch = 0;
    mse::DevBuf x, h, y;
    std::mutex mu;
};

namespace mse {

// core::slice::binary_search_by with cmp(x) = x.partial_cmp(&s) (Rust 1.7x: halve `size`, keep `base`): Ok(p) or Err(p) -> p
__device__ __forceinline__ uint8_t descriptor_bucket(const float* __restrict__ cdf, int cdf_len, float s) {
    size_t size = (size_t)cdf_len, base = 0;
    if (size == 0) return 0;
    while (size > 1) {
        const size_t half = size / 2, mid = base + half;
        base = (cdf[mid] > s) ? base : mid;
        size -= half;
    }
    const float c = cdf[base];
    const size_t r = (c == s) ? base : base + (c < s ? 1 : 0);
    return (uint8_t)r;
}

}  // namespace mse
