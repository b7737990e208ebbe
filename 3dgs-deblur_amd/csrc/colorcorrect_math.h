// colorcorrect_math.h — per-pixel and per-channel math of the colour-corrected evaluation metrics (mip-NeRF 360's
// `color_correct`, as adopted by gsplat's lib_bilagrid and nerfstudio splatfacto's `color_corrected_metrics`), shared by
// csrc/colorcorrect.hip and the host build of tests/host_math/colorcorrect_host.cpp (TEST INFRASTRUCTURE ONLY; same
// arrangement as bilagrid_math.h).
//
// None of the upstream projects is part of the reference tree: the algorithm is recollected, and
// tests/colorcorrect_reference.py restates it in float64.
//
//   inputs   img, ref [H,W,3] float32 in [0,1]; num_iters (5), eps (0.5/255)
//   masks    unclipped(z) = lo <= z <= hi with lo = float(eps), hi = float(1 - eps): float32 compares of stored float32
//            values.  Row mask of output channel c: unclipped(img[c]) & unclipped(x[c]) & unclipped(ref[c]); the first
//            term is taken from the ORIGINAL image in every iteration
//   features a(x) = (r r, r g, r b, g g, g b, b b, r, g, b, 1) of the current image x = (r, g, b), in float64
//   fit      w_c minimises sum_masked (a . w - ref[c])^2: the normal equations G w = h, G = sum a a^T (55 unique sums),
//            h = sum a ref[c] (10 sums), all in float64.  The number of unmasked pixels is G[9][9]
//   solve    Cholesky of the Jacobi-scaled matrix S = D G D, D = diag(G)^-1/2 (unit diagonal), in float64
//   rule     a channel keeps the IDENTITY warp (1 on its own linear feature, 0 elsewhere) for this iteration when it has
//            fewer than kMinCount unmasked pixels, when a diagonal entry of G is not positive, or when a Cholesky pivot of
//            S is not above kPivotTol.  (Upstream's lstsq returns a minimum-norm or all-zero warp there, which turns a
//            black or constant render to zero.)  Pivot k of S is 1 - R^2 of feature k regressed on features 0..k-1:
//            below 1e-10 the float64 normal equations keep fewer than about six digits of w
//   apply    x <- clip(a . [w_0 w_1 w_2], 0, 1) in float64 for every pixel, masked or not, stored as float32
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_CC_HD __host__ __device__ __forceinline__
#else
#define GS_CC_HD inline
#endif

namespace gs {
namespace colorcorrect {

constexpr int kFeatures = 10;
constexpr int kGram = 55;                       // unique entries of the symmetric 10 x 10 matrix, row-major upper triangle
constexpr int kSums = kGram + kFeatures;        // per channel: G (55) then h (10)
constexpr int kMinCount = 10;
constexpr double kPivotTol = 1e-10;

// a pixel as the moments pass stages it: (r, g, b, 1, ref_0, ref_1, ref_2); every term of every sum is a product of four
// of these slots
constexpr int kSlots = 7, kSlotOne = 3, kSlotRef = 4;

GS_CC_HD bool unclipped(float z, float lo, float hi) { return z >= lo && z <= hi; }

// bit c: pixel takes part in the fit of output channel c
GS_CC_HD unsigned row_masks(const float img[3], const float x[3], const float ref[3], float lo, float hi) {
  unsigned m = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (unclipped(img[c], lo, hi) && unclipped(x[c], lo, hi) && unclipped(ref[c], lo, hi)) m |= 1u << c;
  return m;
}

// feature i = slot p * slot q of (r, g, b, 1)
GS_CC_HD void feature_slots(int i, int& p, int& q) {
  const int P[kFeatures] = {0, 0, 0, 1, 1, 2, 0, 1, 2, 3};
  const int Q[kFeatures] = {0, 1, 2, 1, 2, 2, 3, 3, 3, 3};
  p = P[i];
  q = Q[i];
}

GS_CC_HD void features(const float x[3], double a[kFeatures]) {
  const double v[4] = {(double)x[0], (double)x[1], (double)x[2], 1.0};
#pragma unroll
  for (int i = 0; i < kFeatures; ++i) {
    int p, q;
    feature_slots(i, p, q);
    a[i] = v[p] * v[q];                        // exact: the product of two float32 values fits a float64
  }
}

// index of G[i][j], i <= j, in the packed upper triangle
GS_CC_HD int gram_index(int i, int j) { return i * kFeatures - i * (i - 1) / 2 + (j - i); }

// sum k (< kSums) of channel c adds (slot s[0] * slot s[1]) * (slot s[2] * slot s[3]) per unmasked pixel: G[i][j] =
// a_i * a_j for k = gram_index(i, j), h[i] = a_i * (ref_c * 1) for k = kGram + i
GS_CC_HD void sum_slots(int k, int c, int s[4]) {
  if (k >= kGram) {
    feature_slots(k - kGram, s[0], s[1]);
    s[2] = kSlotRef + c;
    s[3] = kSlotOne;
    return;
  }
  int i = 0, first = 0;
  while (k >= first + (kFeatures - i)) { first += kFeatures - i; ++i; }
  feature_slots(i, s[0], s[1]);
  feature_slots(i + (k - first), s[2], s[3]);
}

GS_CC_HD void identity_warp(int c, double* w) {
#pragma unroll
  for (int i = 0; i < kFeatures; ++i) w[i] = (i == 6 + c) ? 1.0 : 0.0;
}

// w of channel c from its kSums sums; L: kFeatures * kFeatures doubles of scratch, d: kFeatures.  False (and the identity
// warp) under the degenerate rule; a NaN anywhere in the sums fails a comparison and lands there too.
GS_CC_HD bool solve_channel(const double* sums, int c, double* L, double* d, double* w) {
  constexpr int n = kFeatures;
  identity_warp(c, w);
  if (!(sums[gram_index(n - 1, n - 1)] >= (double)kMinCount)) return false;
  for (int i = 0; i < n; ++i) {
    const double g = sums[gram_index(i, i)];
    if (!(g > 0.0)) return false;
    d[i] = 1.0 / ::sqrt(g);              // ::sqrt: inside namespace gs a float overload would hide it
  }
  for (int j = 0; j < n; ++j) {
    double s = sums[gram_index(j, j)] * d[j] * d[j];
    for (int k = 0; k < j; ++k) s -= L[j * n + k] * L[j * n + k];
    if (!(s > kPivotTol)) return false;
    const double ljj = ::sqrt(s);
    L[j * n + j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double t = sums[gram_index(j, i)] * d[j] * d[i];
      for (int k = 0; k < j; ++k) t -= L[i * n + k] * L[j * n + k];
      L[i * n + j] = t / ljj;
    }
  }
  for (int i = 0; i < n; ++i) {                 // L y = D h (y in w)
    double t = sums[kGram + i] * d[i];
    for (int k = 0; k < i; ++k) t -= L[i * n + k] * w[k];
    w[i] = t / L[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {            // L^T z = y, w = D z
    double t = w[i];
    for (int k = i + 1; k < n; ++k) t -= L[k * n + i] * w[k];
    w[i] = t / L[i * n + i];
  }
  for (int i = 0; i < n; ++i) w[i] *= d[i];
  return true;
}

// W: the three warps [3][kFeatures]
GS_CC_HD void apply_warp(const float x[3], const double* W, float out[3]) {
  double a[kFeatures];
  features(x, a);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < kFeatures; ++i) v += a[i] * W[c * kFeatures + i];
    out[c] = (float)fmin(fmax(v, 0.0), 1.0);
  }
}

}  // namespace colorcorrect
}  // namespace gs
