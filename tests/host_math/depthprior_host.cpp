// TEST INFRASTRUCTURE ONLY: csrc/depthprior_math.h compiled for the host (tests/test_depthprior_host.py).  The per-pixel
// functions, the moments, the coefficients and the gradient chain are the kernels'; the pixels of a frame are added one
// after the other here.
#include "depthprior_math.h"

namespace dp = gs::depthprior;

extern "C" {

int dph_moments() { return dp::kMoments; }
int dph_stats() { return dp::kStats; }
double dph_degenerate_tol() { return dp::kDegenerateTol; }

// the arguments of gs_depth_prior_loss, host pointers
void dph_depth_prior_loss(int B, int S, int H, int W, const float* depth_acc, const float* alphas, const float* prior,
                          int kind, int space, float min_alpha, float weight, float* loss_out, double* stats_out,
                          float* v_depth_acc, float* v_alphas) {
  const size_t pixels = (size_t)H * W;
  for (int b = 0; b < B; ++b) {
    const size_t frame = (size_t)b * S * pixels;
    dp::Moments m;
    dp::clear_moments(m);
    for (size_t p = 0; p < pixels; ++p) {
      const float d = dp::sample_mean(depth_acc + frame + p, pixels, S);
      const float a = dp::sample_mean(alphas + frame + p, pixels, S);
      const float y = prior[b * pixels + p];
      float x;
      const bool valid = dp::pixel_x(d, a, y, space, min_alpha, &x);
      dp::add_pixel(m, valid, x, y, kind);
    }
    const dp::Coef c = dp::finish(m, kind, (double)weight);
    loss_out[b] = (float)c.loss;
    double* st = stats_out + (size_t)b * dp::kStats;
    st[0] = m.n; st[1] = m.sx; st[2] = m.sy; st[3] = m.sxx; st[4] = m.syy; st[5] = m.sxy; st[6] = m.sabs; st[7] = c.rho;
    for (size_t p = 0; p < pixels; ++p) {
      const float d = dp::sample_mean(depth_acc + frame + p, pixels, S);
      const float a = dp::sample_mean(alphas + frame + p, pixels, S);
      const float y = prior[b * pixels + p];
      float x, vd = 0.0f, va = 0.0f;
      if (dp::pixel_x(d, a, y, space, min_alpha, &x) && !c.degenerate) dp::chain(dp::grad_x(c, x, y), d, a, space, S, &vd, &va);
      for (int s = 0; s < S; ++s) {
        v_depth_acc[frame + (size_t)s * pixels + p] = vd;
        v_alphas[frame + (size_t)s * pixels + p] = va;
      }
    }
  }
}

}  // extern "C"
