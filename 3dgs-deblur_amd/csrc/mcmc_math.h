// mcmc_math.h — per-Gaussian math of the 3DGS-MCMC strategy (Kheradmand et al. 2024), shared by csrc/mcmc.hip and the
// host build of tests/host_math/mcmc_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as gs_math.h).
//
// gsplat is not part of the reference tree: the formulas are recollected from gsplat 1.x `relocation.cu` and
// `strategy/ops.py` (`compute_relocation`, `inject_noise_to_position`); the counter-based generator is Philox4x32-10
// (Salmon et al. 2011, Random123), checked against Random123's known answers.
//
//   noise      delta = Sigma * (z * gate * scaler),  Sigma = R(q / |q|) diag(exp(ls))^2 R^T,
//              gate = 1 / (1 + exp(100 (o - 0.005))), o = sigmoid(logit)      (upstream: op_sigmoid(1 - o, k=100, x0=0.995))
//   relocation o' = 1 - (1 - o)^(1/n),  s' = s * o / D,
//              D = sum_{k=0..n-1} C(n, k+1) (-1)^k o'^(k+1) / sqrt(k+1)       (n co-located copies, clamped to 51)
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_MCMC_HD __host__ __device__ __forceinline__
#else
#define GS_MCMC_HD inline
#endif

namespace gs {
namespace mcmc {

constexpr int kMaxRatio = 51;                  // upstream's binomial table is 51 x 51
constexpr float kGateK = 100.0f;               // steepness of the opacity gate
constexpr float kGateX0 = 0.005f;              // ... and the opacity at which it is 1/2 (1 - 0.995)

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

GS_MCMC_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Philox4x32-10: counter c[4], key (k0, k1) -> four words in c
GS_MCMC_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = mulhi32(kPhiloxM0, c[0]), lo0 = kPhiloxM0 * c[0];
    const uint32_t hi1 = mulhi32(kPhiloxM1, c[2]), lo1 = kPhiloxM1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
}

// the four words of row `row` at step `step` under `seed`: counter (row, 0, step_lo, step_hi), key (seed_lo, seed_hi)
GS_MCMC_HD void row_words(uint32_t row, uint64_t seed, uint64_t step, uint32_t w[4]) {
  w[0] = row; w[1] = 0u; w[2] = (uint32_t)step; w[3] = (uint32_t)(step >> 32);
  philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// three standard normals from four words (Box-Muller): u = (x + 0.5) 2^-32 lies in (0, 1], so ln u is finite and
// |z| <= sqrt(-2 ln 2^-33) = 6.76
GS_MCMC_HD void normals3(const uint32_t w[4], float z[3]) {
  const float k = 2.3283064365386963e-10f;     // 2^-32
  const float u0 = ((float)w[0] + 0.5f) * k, u1 = ((float)w[1] + 0.5f) * k;
  const float u2 = ((float)w[2] + 0.5f) * k, u3 = ((float)w[3] + 0.5f) * k;
  const float two_pi = 6.283185307179586f;
  const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
  z[0] = r0 * cosf(two_pi * u1);
  z[1] = r0 * sinf(two_pi * u1);
  z[2] = r1 * cosf(two_pi * u3);
}

// displacement of one Gaussian from its RAW parameters (log-scales, unnormalised wxyz quaternion, opacity logit) and
// three normals: Sigma * (z * gate * scaler), evaluated as R (s^2 * (R^T v)) — Sigma itself is never formed
GS_MCMC_HD void noise_delta(const float ls[3], const float q[4], float logit, const float z[3], float scaler,
                            float delta[3]) {
  const float o = 1.0f / (1.0f + expf(-logit));
  const float gate = 1.0f / (1.0f + expf(kGateK * (o - kGateX0)));
  const float g = gate * scaler;
  const float v0 = z[0] * g, v1 = z[1] * g, v2 = z[2] * g;
  const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, zz = q[3] * inv;
  const float r00 = 1.0f - 2.0f * (y * y + zz * zz), r01 = 2.0f * (x * y - w * zz), r02 = 2.0f * (x * zz + w * y);
  const float r10 = 2.0f * (x * y + w * zz), r11 = 1.0f - 2.0f * (x * x + zz * zz), r12 = 2.0f * (y * zz - w * x);
  const float r20 = 2.0f * (x * zz - w * y), r21 = 2.0f * (y * zz + w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
  const float s0 = expf(ls[0]), s1 = expf(ls[1]), s2 = expf(ls[2]);
  const float t0 = (r00 * v0 + r10 * v1 + r20 * v2) * (s0 * s0);
  const float t1 = (r01 * v0 + r11 * v1 + r21 * v2) * (s1 * s1);
  const float t2 = (r02 * v0 + r12 * v1 + r22 * v2) * (s2 * s2);
  delta[0] = r00 * t0 + r01 * t1 + r02 * t2;
  delta[1] = r10 * t0 + r11 * t1 + r12 * t2;
  delta[2] = r20 * t0 + r21 * t1 + r22 * t2;
}

// opacity and scale of n co-located copies that together render what one Gaussian (o, s) rendered; n is clamped to
// [1, kMaxRatio].  o' and D are formed in double (1 - (1 - o)^(1/n) cancels to 1e-4 of its operands at small o and
// large n; the alternating sum loses up to two digits); the binomials C(n, k+1) come from the recurrence
// C(n, k+1) = C(n, k) (n - k) / (k + 1), exact in double for n <= 51.
GS_MCMC_HD void relocation(float o, const float s[3], int n, float* new_o, float new_s[3]) {
  n = n < 1 ? 1 : (n > kMaxRatio ? kMaxRatio : n);
  const double od = (double)o;
  const double op = -expm1(log1p(-od) / (double)n);          // 1 - (1 - o)^(1/n)
  double D = 0.0, binom = 1.0, pw = 1.0, sign = 1.0;
  for (int k = 0; k < n; ++k) {
    binom = binom * (double)(n - k) / (double)(k + 1);         // C(n, k+1)
    pw *= op;                                                  // o'^(k+1)
    D += sign * binom * pw / sqrt((double)(k + 1));
    sign = -sign;
  }
  const double coeff = D > 0.0 ? od / D : 1.0;                // o == 0: nothing to preserve, the scale stays
  *new_o = (float)op;
  new_s[0] = (float)((double)s[0] * coeff);
  new_s[1] = (float)((double)s[1] * coeff);
  new_s[2] = (float)((double)s[2] * coeff);
}

}  // namespace mcmc
}  // namespace gs
