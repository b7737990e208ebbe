// TEST INFRASTRUCTURE ONLY: csrc/colorcorrect_math.h compiled for the host (tests/test_colorcorrect_host.py).  The
// per-pixel functions, the slots of every sum and the solve are the kernels'; the sums over pixels run here pixel after
// pixel.
#include <vector>
#include "colorcorrect_math.h"

namespace cc = gs::colorcorrect;

extern "C" {

void ch_features(const float* x, double* a) { cc::features(x, a); }

unsigned ch_row_masks(const float* img, const float* x, const float* ref, double eps) {
  return cc::row_masks(img, x, ref, (float)eps, (float)(1.0 - eps));
}

int ch_gram_index(int i, int j) { return cc::gram_index(i, j); }

// sums [3][kSums] of P pixels, every term formed from its four slots as the moments kernel forms it
void ch_moments(long long P, const float* img, const float* x, const float* ref, double eps, double* sums) {
  const float lo = (float)eps, hi = (float)(1.0 - eps);
  for (int k = 0; k < 3 * cc::kSums; ++k) sums[k] = 0.0;
  for (long long p = 0; p < P; ++p) {
    const float* px = x + 3 * p;
    const float* pr = ref + 3 * p;
    const double v[8] = {px[0], px[1], px[2], 1.0, pr[0], pr[1], pr[2], 0.0};
    const unsigned m = cc::row_masks(img + 3 * p, px, pr, lo, hi);
    for (int c = 0; c < 3; ++c) {
      if (!((m >> c) & 1u)) continue;
      for (int k = 0; k < cc::kSums; ++k) {
        int s[4];
        cc::sum_slots(k, c, s);
        sums[c * cc::kSums + k] += (v[s[0]] * v[s[1]]) * (v[s[2]] * v[s[3]]);
      }
    }
  }
}

int ch_solve(const double* sums, int c, double* w) {
  double L[cc::kFeatures * cc::kFeatures], d[cc::kFeatures];
  return cc::solve_channel(sums, c, L, d, w) ? 1 : 0;
}

// the whole fit of one image pair: out [P,3], warps [num_iters][3][10]
void ch_color_correct(long long P, const float* img, const float* ref, int num_iters, double eps, float* out,
                      double* warps) {
  std::vector<float> x(img, img + 3 * P);
  std::vector<double> sums(3 * cc::kSums);
  for (int it = 0; it < num_iters; ++it) {
    double* W = warps + (size_t)it * 3 * cc::kFeatures;
    ch_moments(P, img, x.data(), ref, eps, sums.data());
    for (int c = 0; c < 3; ++c) ch_solve(sums.data() + c * cc::kSums, c, W + c * cc::kFeatures);
    for (long long p = 0; p < P; ++p) {
      float y[3];
      cc::apply_warp(x.data() + 3 * p, W, y);
      x[3 * p] = y[0]; x[3 * p + 1] = y[1]; x[3 * p + 2] = y[2];
    }
  }
  for (long long i = 0; i < 3 * P; ++i) out[i] = x[i];
}

}  // extern "C"
