// The fixed exponential of the rater (rater.hip) and what derives from it.  Every operation is a correctly rounded f32 operation -- a
// compare, rintf, fmaf, a multiply, an add, a divide -- so the bits are the same on the device, on the host and in numpy
// (tests/rater_ref.py repeats the function with these constants).  No library expf, no fast-math intrinsic: the hardware exponential
// pins no bits (DESIGN.md 3.27 found the same of __fsqrt_rn).
//
//   exp_fixed(x)   x clamped to [-87, 87] (a NaN stays a NaN); n = rintf(x * LOG2E); r = fmaf(n, -LN2_LO, fmaf(n, -LN2_HI, x)) -- LN2_HI
//                  has 11 trailing zero bits, so n * LN2_HI is exact for |n| <= 126 and |r| <= ln2 / 2 up to the rounding of n;
//                  p = the degree-7 Taylor polynomial by Horner, p = fmaf(p, r, c_i) from c_7 down to c_0 = 1; the result is p * 2^n,
//                  exact: -126 <= n <= 126 and the product is a normal number (e^-87 > 2^-126)
//   sig(t)         1 / (1 + exp_fixed(-t)): one add, one divide.  With the clamp it lies in [1.6e-38, 1], never subnormal
//   silu(u)        u * sig(u)
//   silu_grad(u)   s = sig(u); s * (1 + u * (1 - s)): a subtract, a multiply, an add, a multiply, in that order, no fma
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RATER_HD __host__ __device__ inline
#else
#define RATER_HD inline
#endif

namespace mse {

constexpr float RATER_EXP_LO = -87.0f, RATER_EXP_HI = 87.0f;
constexpr float RATER_LOG2E = 1.44269502162933349609375f;         // 0x3FB8AA3B
constexpr float RATER_LN2_HI = 0.693145751953125f;                // 0x3F317200
constexpr float RATER_LN2_LO = 1.42860676533018704503775e-06f;    // 0x35BFBE8E
constexpr float RATER_C2 = 0.5f, RATER_C3 = 0.16666667163372039794921875f, RATER_C4 = 0.0416666679084300994873046875f,
                RATER_C5 = 0.008333333767950534820556640625f, RATER_C6 = 0.001388888922519981861114501953125f,
                RATER_C7 = 0.0001984127011382952332496643066406f;

RATER_HD float exp_fixed(float x) {
    x = x < RATER_EXP_LO ? RATER_EXP_LO : x;
    x = x > RATER_EXP_HI ? RATER_EXP_HI : x;
    const float n = rintf(x * RATER_LOG2E);
    float r = fmaf(n, -RATER_LN2_HI, x);
    r = fmaf(n, -RATER_LN2_LO, r);
    float p = RATER_C7;
    p = fmaf(p, r, RATER_C6);
    p = fmaf(p, r, RATER_C5);
    p = fmaf(p, r, RATER_C4);
    p = fmaf(p, r, RATER_C3);
    p = fmaf(p, r, RATER_C2);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    if (!(n == n)) return n;                                      // a NaN input
    const uint32_t bits = (uint32_t)((int)n + 127) << 23;         // 2^n, 1 <= n + 127 <= 253
    float scale;
    memcpy(&scale, &bits, 4);
    return p * scale;
}

RATER_HD float rater_sig(float t) {
    const float d = 1.0f + exp_fixed(-t);
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(1.0f, d);   // the correctly rounded quotient whatever the build's division mode
#else
    return 1.0f / d;
#endif
}

RATER_HD float rater_silu(float u) { return u * rater_sig(u); }

RATER_HD float rater_silu_grad(float u) {
    const float s = rater_sig(u);
    const float a = 1.0f - s;
    const float b = u * a;
    const float c = 1.0f + b;
    return s * c;
}

}  // namespace mse
