// TEST INFRASTRUCTURE ONLY: csrc/normal_math.h compiled for the host (tests/test_normals_host.py).  The per-pixel
// functions, the sums, the coefficients and the gradient chain are the kernels'; the pixels of a frame are visited one
// after the other here, on whole-frame arrays instead of tiles.
#include <algorithm>
#include <vector>

#include "normal_math.h"

namespace nm = gs::normal;
namespace dp = gs::depthprior;

extern "C" {

int nmh_stats() { return nm::kStats; }
float nmh_min_l2() { return nm::kMinL2; }

// the arguments of gs_normal_loss, host pointers; prior, guide and normals_out may be null
void nmh_normal_loss(int B, int S, int H, int W, const float* depth_acc, const float* alphas, const float* intrins,
                     const float* prior, const float* guide, float prior_weight, float smooth_weight, float edge_beta,
                     float min_alpha, float* loss_out, double* stats_out, float* normals_out, float* v_depth_acc,
                     float* v_alphas) {
  const size_t pixels = (size_t)H * W;
  if (!(edge_beta > 0.0f)) guide = nullptr;
  // one ring of zeros around the frame, so that every neighbour can be addressed
  const int PW = W + 2, PH = H + 2;
  std::vector<float> d((size_t)PW * PH), a((size_t)PW * PH), n((size_t)PW * PH * 3);
  std::vector<double> vt((size_t)PW * PH * 6);
  for (int b = 0; b < B; ++b) {
    const size_t frame = (size_t)b * S * pixels, image = (size_t)b * pixels;
    const float* K = intrins + b * 4;
    const float* pr = prior ? prior + image * 3 : nullptr;
    const float* gd = guide ? guide + image * 3 : nullptr;
    std::fill(d.begin(), d.end(), 0.0f);
    std::fill(a.begin(), a.end(), 0.0f);
    std::fill(n.begin(), n.end(), 0.0f);
    std::fill(vt.begin(), vt.end(), 0.0);
    auto at = [&](int u, int v) { return (size_t)(v + 1) * PW + (u + 1); };
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        d[at(u, v)] = dp::sample_mean(depth_acc + frame + (size_t)v * W + u, pixels, S);
        a[at(u, v)] = dp::sample_mean(alphas + frame + (size_t)v * W + u, pixels, S);
      }
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u)
        nm::normal_at(d.data() + at(u, v), a.data() + at(u, v), PW, u, v, H, W, K, min_alpha, n.data() + at(u, v) * 3);
    nm::Sums m;
    nm::clear_sums(m);
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const size_t p = (size_t)v * W + u;
        const float* np_ = n.data() + at(u, v) * 3;
        if (normals_out)
          for (int k = 0; k < 3; ++k) normals_out[(image + p) * 3 + k] = np_[k];
        if (!nm::defined(np_)) continue;
        nm::add_defined(m);
        float unit[3];
        if (pr && nm::prior_unit(pr + p * 3, unit)) nm::add_prior(m, np_, unit);
        const float* nr = n.data() + at(u + 1, v) * 3;
        const float* nd = n.data() + at(u, v + 1) * 3;
        if (nm::defined(nr)) nm::add_pair(m, np_, nr, gd ? nm::pair_weight(gd + p * 3, gd + (p + 1) * 3, edge_beta) : 1.0f);
        if (nm::defined(nd)) nm::add_pair(m, np_, nd, gd ? nm::pair_weight(gd + p * 3, gd + (p + W) * 3, edge_beta) : 1.0f);
      }
    const nm::Coef c = nm::finish(m, (double)prior_weight, (double)smooth_weight);
    loss_out[b] = (float)c.loss;
    double* st = stats_out + (size_t)b * nm::kStats;
    st[0] = m.n_def; st[1] = m.np; st[2] = m.sp; st[3] = m.ns; st[4] = m.ss; st[5] = m.sg;
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const size_t h = at(u, v), p = (size_t)v * W + u;
        const float* np_ = n.data() + h * 3;
        if (!nm::defined(np_)) continue;
        float unit[3] = {0.0f, 0.0f, 0.0f};
        if (pr) nm::prior_unit(pr + p * 3, unit);
        double pair_sum[3] = {0.0, 0.0, 0.0};
        const size_t hq[4] = {h - 1, h + 1, h - PW, h + PW};
        const size_t pq[4] = {p - 1, p + 1, p - W, p + W};
        for (int j = 0; j < 4; ++j) {
          const float* nq = n.data() + hq[j] * 3;
          if (!nm::defined(nq)) continue;
          const float g = gd ? nm::pair_weight(gd + p * 3, gd + pq[j] * 3, edge_beta) : 1.0f;
          for (int k = 0; k < 3; ++k) pair_sum[k] += (double)g * (double)nq[k];
        }
        double vn[3];
        nm::grad_normal(c, unit, pair_sum, vn);
        nm::Geom g;
        nm::geometry(u, v, K, d[h - 1] / a[h - 1], d[h + 1] / a[h + 1], d[h - PW] / a[h - PW], d[h + PW] / a[h + PW], g);
        nm::grad_tangents(g, np_, vn, vt.data() + h * 6, vt.data() + h * 6 + 3);
      }
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const size_t h = at(u, v), p = (size_t)v * W + u;
        float vd = 0.0f, va = 0.0f;
        if (nm::has_z(d[h], a[h], min_alpha)) {
          const double* l = vt.data() + (h - 1) * 6;
          const double* r = vt.data() + (h + 1) * 6;
          const double* up = vt.data() + (h - PW) * 6 + 3;
          const double* dn = vt.data() + (h + PW) * 6 + 3;
          const double vP[3] = {((l[0] - r[0]) + up[0]) - dn[0], ((l[1] - r[1]) + up[1]) - dn[1], ((l[2] - r[2]) + up[2]) - dn[2]};
          dp::chain(nm::grad_z(u, v, K, vP), d[h], a[h], dp::kDepth, S, &vd, &va);
        }
        for (int s = 0; s < S; ++s) {
          v_depth_acc[frame + (size_t)s * pixels + p] = vd;
          v_alphas[frame + (size_t)s * pixels + p] = va;
        }
      }
  }
}

}  // extern "C"
