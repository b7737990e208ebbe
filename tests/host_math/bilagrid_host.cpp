// TEST INFRASTRUCTURE ONLY: csrc/bilagrid_math.h compiled for the host (tests/test_bilagrid_host.py).  The per-pixel
// functions are the kernels'; the sums over pixels run here in double, pixel after pixel.
#include <vector>
#include "bilagrid_math.h"

namespace bg = gs::bilagrid;

namespace {
struct GlobalGrid {
  const float* g;      // one image's grid [12, L, GH, GW]
  int GW, GH, L;
  float operator()(int z, int y, int x, int c) const { return g[(((size_t)c * L + z) * GH + y) * GW + x]; }
};
}  // namespace

extern "C" {

void bh_slice_fwd(int B, int H, int W, int G, int GW, int GH, int L, const float* grids, const int* grid_idx,
                  const float* rgb, float* out) {
  const size_t gsz = (size_t)bg::kChannels * L * GH * GW;
  for (int b = 0; b < B; ++b) {
    const GlobalGrid v{grids + gsz * grid_idx[b], GW, GH, L};
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t px = (((size_t)b * H + y) * W + x) * 3;
        bg::slice_pixel(x, y, W, H, rgb + px, GW, GH, L, v, out + px);
      }
  }
  (void)G;
}

void bh_slice_bwd(int B, int H, int W, int G, int GW, int GH, int L, const float* grids, const int* grid_idx,
                  const float* rgb, const float* v_out, float* v_rgb, float* v_grids) {
  const size_t gsz = (size_t)bg::kChannels * L * GH * GW;
  std::vector<double> acc(gsz * G, 0.0);
  for (int b = 0; b < B; ++b) {
    const GlobalGrid v{grids + gsz * grid_idx[b], GW, GH, L};
    double* a = acc.data() + gsz * grid_idx[b];
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t px = (((size_t)b * H + y) * W + x) * 3;
        const bg::Cell k = bg::locate(x, y, W, H, rgb + px, GW, GH, L);
        float a0[bg::kChannels], a1[bg::kChannels], A[bg::kChannels], vA[bg::kChannels];
        bg::interp_slices(k, v, a0, a1);
        bg::blend_slices(a0, a1, k.fz, A);
        bg::affine_grad(v_out + px, rgb + px, vA);
        bg::rgb_grad(A, a0, a1, vA, v_out + px, L, k.zin, v_rgb + px);
        for (int dz = 0; dz < 2; ++dz)
          for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
              const float w = (dz ? k.fz : 1.0f - k.fz) * (dy ? k.fy : 1.0f - k.fy) * (dx ? k.fx : 1.0f - k.fx);
              for (int c = 0; c < bg::kChannels; ++c)
                a[(((size_t)c * L + k.z0 + dz) * GH + k.y0 + dy) * GW + k.x0 + dx] += (double)(w * vA[c]);
            }
      }
  }
  for (size_t i = 0; i < acc.size(); ++i) v_grids[i] = (float)acc[i];
}

// value (double) and gradient of weight * tv(grids); v_grids += weight * d tv
double bh_tv(int G, int GW, int GH, int L, const float* grids, float weight, float* v_grids) {
  const long long planes = (long long)G * bg::kChannels;
  const float sx = bg::tv_axis_scale(planes * L * GH * (GW - 1));
  const float sy = bg::tv_axis_scale(planes * L * (GH - 1) * GW);
  const float sz = bg::tv_axis_scale(planes * (L - 1) * GH * GW);
  const long long n = planes * L * GH * GW, sY = GW, sZ = (long long)GW * GH;
  double total = 0.0;
  for (long long e = 0; e < n; ++e) {
    const int x = (int)(e % GW), y = (int)((e / GW) % GH), z = (int)((e / sZ) % L);
    const bool hpx = x > 0, hnx = x + 1 < GW, hpy = y > 0, hny = y + 1 < GH, hpz = z > 0, hnz = z + 1 < L;
    float value, grad;
    bg::tv_element(grids[e], hpx, hpx ? grids[e - 1] : 0.0f, hnx, hnx ? grids[e + 1] : 0.0f, hpy,
                   hpy ? grids[e - sY] : 0.0f, hny, hny ? grids[e + sY] : 0.0f, hpz, hpz ? grids[e - sZ] : 0.0f, hnz,
                   hnz ? grids[e + sZ] : 0.0f, sx, sy, sz, &value, &grad);
    total += (double)value;
    if (v_grids) v_grids[e] += weight * grad;
  }
  return (double)weight * total;
}

float bh_identity_channel(int c) { return bg::identity_channel(c); }

}  // extern "C"
