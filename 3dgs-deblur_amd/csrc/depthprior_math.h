// depthprior_math.h — scale- and shift-invariant depth-prior loss (depthprior.py): 1 - Pearson(rendered, prior), the
// correlation loss of the depth-regularised 3DGS methods for sparse or casual captures (FSGS, SparseGS; recollected, none
// of them is part of the reference tree), and an L1 of the same form.  Shared by csrc/depthprior.hip and the host build of
// tests/host_math/depthprior_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as colorcorrect_math.h and blur_math.h).
// Compile with -ffp-contract=off: every float32 operation below rounds on its own.
//
//   inputs   per frame depth_acc [S,H,W] (the compositor's per-sample sums of weight * camera-space depth), alphas
//            [S,H,W], prior [H,W] (0: no value); kind, space, min_alpha >= 0, weight
//   pixel    d = (((acc[0] + acc[1]) + ...) + acc[S-1]) / float(S), a likewise from alphas: float32, in this order
//   valid    prior > 0 && a > min_alpha, and d > 0 as well in disparity space
//   x, y     x = d / a (depth space) or a / d (disparity space), float32; y = prior
//   sums     over the valid pixels, float64, of the widened float32 values (every product is exact): n, sum x, sum y,
//            sum x x, sum y y, sum x y, and sum |x - y| for the L1
//   pearson  vx = n sxx - sx sx, vy = n syy - sy sy, cov = n sxy - sx sy, rho = cov / sqrt(vx vy), loss = weight (1 - rho)
//            d loss / d x_i = -weight [(n y_i - sy) / sqrt(vx vy) - rho (n x_i - sx) / vx]
//            DEGENERATE (a definition, not a tolerance: a constant render or a constant prior has no correlation):
//            n < 2, or vx <= 1e-12 n sxx, or vy <= 1e-12 n syy -> loss 0 and every gradient exactly 0
//   l1       loss = weight sum |x - y| / max(n, 1), d loss / d x_i = weight sign(x_i - y_i) / n
//   chain    float64, rounded once on store: depth space dx/dd = 1 / a, dx/da = -d / a^2; disparity space dx/da = 1 / d,
//            dx/dd = -a / d^2; v_depth_acc[s] = (d loss / d d) / S and v_alphas[s] = (d loss / d a) / S for every s;
//            exact zeros at invalid pixels
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_DP_HD __host__ __device__ __forceinline__
#else
#define GS_DP_HD inline
#endif

namespace gs {
namespace depthprior {

constexpr int kPearson = 0, kL1 = 1;            // kind
constexpr int kDepth = 0, kDisparity = 1;       // space
constexpr int kMoments = 7;                     // n, sx, sy, sxx, syy, sxy, sabs
constexpr int kStats = 8;                       // the moments, then rho (pearson; 0 when degenerate or for the L1)
constexpr double kDegenerateTol = 1e-12;

struct Moments {
  double n, sx, sy, sxx, syy, sxy, sabs;
};

GS_DP_HD void clear_moments(Moments& m) { m.n = m.sx = m.sy = m.sxx = m.syy = m.sxy = m.sabs = 0.0; }

GS_DP_HD void add_moments(Moments& m, const Moments& o) {
  m.n += o.n; m.sx += o.sx; m.sy += o.sy; m.sxx += o.sxx; m.syy += o.syy; m.sxy += o.sxy; m.sabs += o.sabs;
}

// mean over the S samples of one pixel; plane: elements between two samples
GS_DP_HD float sample_mean(const float* p, size_t plane, int S) {
  float sum = p[0];
  for (int s = 1; s < S; ++s) sum = sum + p[(size_t)s * plane];
  return sum / (float)S;
}

// validity and x of one pixel
GS_DP_HD bool pixel_x(float d, float a, float prior, int space, float min_alpha, float* x) {
  const bool valid = prior > 0.0f && a > min_alpha && (space == kDepth || d > 0.0f);
  *x = valid ? (space == kDepth ? d / a : a / d) : 0.0f;
  return valid;
}

GS_DP_HD void add_pixel(Moments& m, bool valid, float xf, float yf, int kind) {
  if (!valid) return;
  const double x = (double)xf, y = (double)yf;
  m.n += 1.0; m.sx += x; m.sy += y; m.sxx += x * x; m.syy += y * y; m.sxy += x * y;
  if (kind == kL1) m.sabs += fabs(x - y);
}

// what the gradient of every pixel of a frame shares
struct Coef {
  int kind;
  bool degenerate;
  double n, sx, sy, vx, root, rho, weight, loss;
};

GS_DP_HD Coef finish(const Moments& m, int kind, double weight) {
  Coef c;
  c.kind = kind; c.n = m.n; c.sx = m.sx; c.sy = m.sy; c.weight = weight;
  c.vx = c.root = c.rho = c.loss = 0.0;
  if (kind == kL1) {
    c.degenerate = !(m.n >= 1.0);
    c.loss = weight * m.sabs / (m.n > 1.0 ? m.n : 1.0);
    return c;
  }
  const double vx = m.n * m.sxx - m.sx * m.sx, vy = m.n * m.syy - m.sy * m.sy;
  // written so that a NaN in the sums lands in the degenerate branch too
  c.degenerate = !(m.n >= 2.0 && vx > kDegenerateTol * m.n * m.sxx && vy > kDegenerateTol * m.n * m.syy);
  if (c.degenerate) return c;
  c.vx = vx;
  c.root = ::sqrt(vx * vy);               // ::sqrt: inside namespace gs a float overload would hide it
  c.rho = (m.n * m.sxy - m.sx * m.sy) / c.root;
  c.loss = weight * (1.0 - c.rho);
  return c;
}

// d loss / d x of one valid pixel
GS_DP_HD double grad_x(const Coef& c, float xf, float yf) {
  if (c.degenerate) return 0.0;
  const double x = (double)xf, y = (double)yf;
  if (c.kind == kL1) {
    const double e = x - y;
    return e > 0.0 ? c.weight / c.n : (e < 0.0 ? -(c.weight / c.n) : 0.0);
  }
  return -c.weight * ((c.n * y - c.sy) / c.root - c.rho * (c.n * x - c.sx) / c.vx);
}

// d loss / d x -> what every one of the S samples of the pixel receives
GS_DP_HD void chain(double g, float df, float af, int space, int S, float* v_depth_acc, float* v_alphas) {
  const double d = (double)df, a = (double)af;
  double gd, ga;
  if (space == kDepth) {
    gd = g / a;
    ga = -(g * d) / (a * a);
  } else {
    ga = g / d;
    gd = -(g * a) / (d * d);
  }
  *v_depth_acc = (float)(gd / (double)S);
  *v_alphas = (float)(ga / (double)S);
}

}  // namespace depthprior
}  // namespace gs
