// fp32 digamma / trigamma / lgamma for positive arguments, usable on the host and on the device (the hierarchical KL of
// bt_kl_hier.hip evaluates them at a = exp(log_a_q); bt_special_eval runs the same code on the CPU).
//
//   x >= 6: the asymptotic series,                      psi(x)  = ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) + 1/(240x^8)
//                                                       psi'(x) = 1/x + 1/(2x^2) + 1/(6x^3) - 1/(30x^5) + 1/(42x^7) - 1/(30x^9)
//           (first omitted term at x = 6: 1e-11 and 2e-10 -- below half an ulp of the result);
//   x <  6: six steps of the recurrence to y = x + 6,   psi(x)  = psi(y)  - sum_{k<6} 1/(x+k),
//                                                       psi'(x) = psi'(y) + sum_{k<6} 1/(x+k)^2
//           on the six reciprocals themselves (no common denominator: 1/x stays exact to an ulp however small x is).
// The compile flags (-ffp-contract=off on both sides) keep every product and sum a rounded fp32 operation.
// Arguments are > 0 (exp of something); 0 gives -inf / +inf, like the functions' limits.
#pragma once
#include <math.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define BT_SPECIAL_RCP(x) __builtin_amdgcn_rcpf(x)      // 1 ulp
#else
#define BT_SPECIAL_RCP(x) (1.0f / (x))
#endif
#if defined(__HIPCC__)
#define BT_SPECIAL_FN __host__ __device__ __forceinline__
#else
#define BT_SPECIAL_FN inline
#endif

namespace bt {

constexpr float kSpecialShift = 6.0f;      // the recurrence threshold AND its length: x < 6 is evaluated at x + 6

// psi(y) - ln y for y >= 6
BT_SPECIAL_FN float digamma_tail(float w /* 1/y */) {
  const float w2 = w * w;
  const float p = 0.083333333333f - w2 * (0.0083333333333f - w2 * (0.003968253968f - w2 * 0.004166666667f));
  return -(0.5f * w) - w2 * p;
}

// psi'(y) - 1/y for y >= 6
BT_SPECIAL_FN float trigamma_tail(float w /* 1/y */) {
  const float w2 = w * w;
  return w2 * (0.5f + w * (0.166666666667f + w2 * (-0.033333333333f + w2 * (0.0238095238095f + w2 * -0.033333333333f))));
}

BT_SPECIAL_FN float digamma(float x) {
  if (x >= kSpecialShift) return logf(x) + digamma_tail(BT_SPECIAL_RCP(x));
  const float y = x + kSpecialShift;
  const float s01 = BT_SPECIAL_RCP(x) + BT_SPECIAL_RCP(x + 1.0f);
  const float s23 = BT_SPECIAL_RCP(x + 2.0f) + BT_SPECIAL_RCP(x + 3.0f);
  const float s45 = BT_SPECIAL_RCP(x + 4.0f) + BT_SPECIAL_RCP(x + 5.0f);
  return (logf(y) + digamma_tail(BT_SPECIAL_RCP(y))) - ((s45 + s23) + s01);
}

// psi'(x) and x psi'(x) - 1. The second is what the gradient of the hierarchical KL needs: at large x, x psi'(x) -> 1 and
// (x - c) psi'(x) - 1 formed from psi' would cancel to nothing; here it is 1/(2x) + 1/(6x^2) - ... to full relative accuracy.
// Small x: x psi'(x) - 1 = x sum_{k<6} 1/(x+k)^2 + x (psi'(y) - 1/y) - 6/y, with x (1/x)^2 formed as (x/x)(1/x): no overflow
// before psi' itself overflows.
BT_SPECIAL_FN void trigamma_pair(float x, float& psi1, float& x_psi1_m1) {
  if (x >= kSpecialShift) {
    const float w = BT_SPECIAL_RCP(x);
    const float t = trigamma_tail(w);
    psi1 = w + t;
    x_psi1_m1 = x * t;
    return;
  }
  const float y = x + kSpecialShift;
  const float r0 = BT_SPECIAL_RCP(x), r1 = BT_SPECIAL_RCP(x + 1.0f), r2 = BT_SPECIAL_RCP(x + 2.0f);
  const float r3 = BT_SPECIAL_RCP(x + 3.0f), r4 = BT_SPECIAL_RCP(x + 4.0f), r5 = BT_SPECIAL_RCP(x + 5.0f);
  const float q15 = ((r5 * r5 + r4 * r4) + (r3 * r3 + r2 * r2)) + r1 * r1;      // smallest first
  const float w = BT_SPECIAL_RCP(y);
  const float t = trigamma_tail(w);
  psi1 = ((w + t) + q15) + r0 * r0;
  x_psi1_m1 = ((x * (t + q15)) - kSpecialShift * w) + (x * r0) * r0;
}

BT_SPECIAL_FN float trigamma(float x) {
  float p, q;
  trigamma_pair(x, p, q);
  return p;
}

// ln Gamma(x): the C library's / the device library's lgammaf (both hold a few ulps over the whole range, also at the zeros 1 and 2).
BT_SPECIAL_FN float lgamma_pos(float x) { return lgammaf(x); }

}  // namespace bt
