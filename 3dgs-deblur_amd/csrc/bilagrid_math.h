// bilagrid_math.h — per-pixel and per-vertex math of the bilateral-grid colour correction (Chen et al. 2007 "Real-time
// edge-aware image processing with the bilateral grid"; as a per-image learned correction: Wang et al. 2024 "Bilateral
// guided radiance field processing"), shared by csrc/bilagrid.hip and the host build of
// tests/host_math/bilagrid_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as mcmc_math.h).
//
// Neither gsplat nor nerfstudio is part of the reference tree: the formulas are recollected from gsplat's
// `lib_bilagrid.py` (`slice`, `total_variation_loss`, `color_correct` is not used) and nerfstudio splatfacto's
// `use_bilateral_grid` / `_apply_bilateral_grid`.  Upstream evaluates the lookup with a 5-D
// F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True); the direct form below is the same function
// (tests/bilagrid_reference.py IS that grid_sample, in float64).
//
//   grids   [G, 12, L, GH, GW]; the 12 channels are a row-major 3x4 affine [A | b], identity at initialisation
//   sample  pixel (x, y) of an H x W image with colour rgb looks its image's grid up at
//             u = (x + 0.5) / W -> GW axis,  v = (y + 0.5) / H -> GH axis,  g = 0.299 r + 0.587 g + 0.114 b -> L axis
//           each coordinate c clamped to [0, 1] ("border"), position c * (n - 1) ("align_corners"), trilinear
//   apply   out = A rgb + b
//   grads   the 8 x 12 sampled vertices (weight * v_out (x) [rgb, 1]); rgb through A (A^T v_out); rgb through the guide:
//           (L - 1) * sum_c vA_c * (slice z0+1 - slice z0)_c * (0.299, 0.587, 0.114), zero where g left (0, 1)
//   tv      2 * (m_x + m_y + m_z), m_a = mean over images, channels and positions of the squared forward difference
//           along lattice axis a
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_BG_HD __host__ __device__ __forceinline__
#else
#define GS_BG_HD inline
#endif

namespace gs {
namespace bilagrid {

constexpr int kChannels = 12;                                  // row-major 3x4 [A | b]
constexpr int kDefaultGW = 16, kDefaultGH = 16, kDefaultL = 8; // (GW, GH, L) of SplatfactoDeblurConfig.grid_shape
constexpr float kLumaR = 0.299f, kLumaG = 0.587f, kLumaB = 0.114f;   // Rec. 601 luma: the guide
constexpr float kTvScale = 2.0f;                               // tv = kTvScale * (m_x + m_y + m_z)

// identity transform: 1 on the diagonal of A, 0 elsewhere
GS_BG_HD float identity_channel(int c) { return (c == 0 || c == 5 || c == 10) ? 1.0f : 0.0f; }

// centre of pixel i of an axis of `size` pixels, in [0, 1]
GS_BG_HD float pixel_coord(int i, int size) { return ((float)i + 0.5f) / (float)size; }

GS_BG_HD float luma(const float rgb[3]) { return kLumaR * rgb[0] + kLumaG * rgb[1] + kLumaB * rgb[2]; }

// coordinate c on an axis of n >= 2 vertices: cell i0 in [0, n-2] and fraction f in [0, 1] of c clamped to [0, 1];
// `inside`: c lies strictly inside (0, 1) — only there does the position follow c (border padding's gradient rule).
// A NaN coordinate lands in cell 0 with f = 0.
GS_BG_HD void axis_cell(float c, int n, int& i0, float& f, bool& inside) {
  const float cc = fminf(fmaxf(c, 0.0f), 1.0f);
  const float p = cc * (float)(n - 1);
  int i = (int)p;
  if (i > n - 2) i = n - 2;
  if (i < 0) i = 0;
  i0 = i;
  f = p - (float)i;
  inside = (c > 0.0f) && (c < 1.0f);
}

struct Cell {
  int x0, y0, z0;       // lower vertex of the sampled cell
  float fx, fy, fz;     // fractions inside it
  bool zin;             // the guide was not clamped
};

GS_BG_HD Cell locate(int x, int y, int W, int H, const float rgb[3], int GW, int GH, int L) {
  Cell k;
  bool unused;
  axis_cell(pixel_coord(x, W), GW, k.x0, k.fx, unused);
  axis_cell(pixel_coord(y, H), GH, k.y0, k.fy, unused);
  axis_cell(luma(rgb), L, k.z0, k.fz, k.zin);
  return k;
}

// bilinear (x, y) interpolation of the two L-slices z0 and z0 + 1 of the cell; v(z, y, x, c) reads one grid value
template <class V>
GS_BG_HD void interp_slices(const Cell& k, V&& v, float a0[kChannels], float a1[kChannels]) {
  const float w00 = (1.0f - k.fx) * (1.0f - k.fy), w01 = k.fx * (1.0f - k.fy);
  const float w10 = (1.0f - k.fx) * k.fy, w11 = k.fx * k.fy;
#pragma unroll
  for (int c = 0; c < kChannels; ++c) {
    a0[c] = w00 * v(k.z0, k.y0, k.x0, c) + w01 * v(k.z0, k.y0, k.x0 + 1, c) + w10 * v(k.z0, k.y0 + 1, k.x0, c) +
            w11 * v(k.z0, k.y0 + 1, k.x0 + 1, c);
    a1[c] = w00 * v(k.z0 + 1, k.y0, k.x0, c) + w01 * v(k.z0 + 1, k.y0, k.x0 + 1, c) +
            w10 * v(k.z0 + 1, k.y0 + 1, k.x0, c) + w11 * v(k.z0 + 1, k.y0 + 1, k.x0 + 1, c);
  }
}

GS_BG_HD void blend_slices(const float a0[kChannels], const float a1[kChannels], float fz, float A[kChannels]) {
#pragma unroll
  for (int c = 0; c < kChannels; ++c) A[c] = (1.0f - fz) * a0[c] + fz * a1[c];
}

GS_BG_HD void apply_affine(const float A[kChannels], const float rgb[3], float out[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = A[4 * i] * rgb[0] + A[4 * i + 1] * rgb[1] + A[4 * i + 2] * rgb[2] + A[4 * i + 3];
}

// d loss / d (interpolated affine): v_out (x) [rgb, 1]
GS_BG_HD void affine_grad(const float v_out[3], const float rgb[3], float vA[kChannels]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    vA[4 * i] = v_out[i] * rgb[0];
    vA[4 * i + 1] = v_out[i] * rgb[1];
    vA[4 * i + 2] = v_out[i] * rgb[2];
    vA[4 * i + 3] = v_out[i];
  }
}

// d loss / d rgb: through A, and through the guide
GS_BG_HD void rgb_grad(const float A[kChannels], const float a0[kChannels], const float a1[kChannels],
                       const float vA[kChannels], const float v_out[3], int L, bool zin, float v_rgb[3]) {
  float dz = 0.0f;
#pragma unroll
  for (int c = 0; c < kChannels; ++c) dz += vA[c] * (a1[c] - a0[c]);
  dz = zin ? dz * (float)(L - 1) : 0.0f;
  const float lw[3] = {kLumaR, kLumaG, kLumaB};
#pragma unroll
  for (int j = 0; j < 3; ++j) v_rgb[j] = A[j] * v_out[0] + A[4 + j] * v_out[1] + A[8 + j] * v_out[2] + dz * lw[j];
}

// one pixel forward; v as in interp_slices
template <class V>
GS_BG_HD void slice_pixel(int x, int y, int W, int H, const float rgb[3], int GW, int GH, int L, V&& v, float out[3]) {
  const Cell k = locate(x, y, W, H, rgb, GW, GH, L);
  float a0[kChannels], a1[kChannels], A[kChannels];
  interp_slices(k, v, a0, a1);
  blend_slices(a0, a1, k.fz, A);
  apply_affine(A, rgb, out);
}

// ---- total variation ------------------------------------------------------------------------------------------------
// what ONE lattice value contributes: to the value, its forward differences (towards +x, +y, +z where that neighbour
// exists); to its own gradient, every difference it takes part in.  sx / sy / sz = kTvScale / (number of differences
// along that axis over the whole tensor), 0 for an axis without differences.
GS_BG_HD void tv_element(float v, bool has_px, float px, bool has_nx, float nx, bool has_py, float py, bool has_ny,
                         float ny, bool has_pz, float pz, bool has_nz, float nz, float sx, float sy, float sz,
                         float* value, float* grad) {
  const float dxn = has_nx ? nx - v : 0.0f, dyn = has_ny ? ny - v : 0.0f, dzn = has_nz ? nz - v : 0.0f;
  const float dxp = has_px ? v - px : 0.0f, dyp = has_py ? v - py : 0.0f, dzp = has_pz ? v - pz : 0.0f;
  *value = sx * dxn * dxn + sy * dyn * dyn + sz * dzn * dzn;
  *grad = 2.0f * (sx * (dxp - dxn) + sy * (dyp - dyn) + sz * (dzp - dzn));
}

GS_BG_HD float tv_axis_scale(long long differences) {
  return differences > 0 ? (float)((double)kTvScale / (double)differences) : 0.0f;
}

}  // namespace bilagrid
}  // namespace gs
