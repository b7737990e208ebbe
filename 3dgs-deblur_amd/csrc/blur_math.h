// blur_math.h — predicted per-frame blur of a point cloud seen by moving cameras (blurscore.py, csrc/blur.hip): how many
// pixels the paper's first-order motion model smears a frame by, and how far its rolling shutter shears it.  Plain
// host+device C++ (GS_HD): tests/host_math/blur_host.cpp compiles this very file with g++.
//
// For frame f (world-to-camera V, OpenCV axes; body twist lin, ang in that camera frame; fx fy cx cy; exposure E, readout
// T) and point p, every operation rounded to fp32 (no fused multiply-add: built with -ffp-contract=off):
//   pc    = V p                      pc.x = ((V0 p.x + V1 p.y) + V2 p.z) + V3, rows 1 and 2 alike
//   rz    = 1 / pc.z
//   (u,v) = ((fx pc.x) rz + cx, (fy pc.y) rz + cy)
//   pv    = pixel_velocity(pc, jx = pc.x, jy = pc.y, rz, fx, fy, lin, ang)          (gs_math.h, the renderer's own)
//   mag   = sqrt(pv.x pv.x + pv.y pv.y)
//   blur  = E mag                    the motion-blur streak of that point, pixels
//   skew  = (T mag) |v / H - 1/2|    how far the rolling shutter moves the point's row, pixels
// The pair is VISIBLE iff pc.z > clip and 0 <= u < W and 0 <= v < H.  Per frame, over its visible pairs:
//   count, mean_blur = sum blur / count, rms_blur = sqrt(sum blur^2 / count), max_blur, mean_skew = sum skew / count,
// all 0 when count == 0.  The three sums are float64 (blur^2 is squared in float64), the quotients and the root are
// float64, rounded to fp32 once.
//
// The sums' order is fixed by N alone: the cloud is cut into chunks of kChunk points; inside a chunk a thread adds its
// points in index order, the 64 lanes of a wave are added in a butterfly (add_partial is commutative bit for bit, so
// every lane holds the same value), the waves of the chunk in order, the chunks in a second pass (64 interleaved parts
// per frame, then the same butterfly).  No atomics.  The host build adds pair after pair instead: the tests compare
// both with a float64 reference, not with each other.
#pragma once
#include "gs_math.h"

namespace gs {
namespace blur {

constexpr int kChunk = 1024;          // points per pass-1 workgroup: one row of partials per (chunk, frame)
constexpr int kFrameGroup = 32;       // frames a pass-1 workgroup loops over with its points held in registers
constexpr float kDefaultClip = 0.01f; // the projection's near plane

// what pass 1 keeps per (chunk, frame) and pass 2 adds up
struct Partial {
  double sum_blur, sum_sq, sum_skew;
  float max_blur;
  int count;
};

GS_HD void clear_partial(Partial& a) {
  a.sum_blur = 0.0; a.sum_sq = 0.0; a.sum_skew = 0.0; a.max_blur = 0.f; a.count = 0;
}

GS_HD void add_partial(Partial& a, const Partial& b) {
  a.sum_blur += b.sum_blur; a.sum_sq += b.sum_sq; a.sum_skew += b.sum_skew;
  a.max_blur = a.max_blur > b.max_blur ? a.max_blur : b.max_blur;
  a.count += b.count;
}

// one frame's constants, as the C ABI passes them
struct Frame {
  const float* V;      // 16, row-major world-to-camera (the last row is not read)
  const float* lin;    // 3
  const float* ang;    // 3
  float fx, fy, cx, cy, E, T;
};

// blur and skew of one (frame, point) pair -> visible?
GS_HD bool pair_blur(const Frame& f, const float p[3], float W, float H, float clip, float* blur, float* skew) {
  const float* V = f.V;
  const float pc[3] = {((V[0] * p[0] + V[1] * p[1]) + V[2] * p[2]) + V[3],
                       ((V[4] * p[0] + V[5] * p[1]) + V[6] * p[2]) + V[7],
                       ((V[8] * p[0] + V[9] * p[1]) + V[10] * p[2]) + V[11]};
  const float rz = 1.f / pc[2];
  const float u = (f.fx * pc[0]) * rz + f.cx;
  const float v = (f.fy * pc[1]) * rz + f.cy;
  float pv[2];
  pixel_velocity(pc, pc[0], pc[1], rz, f.fx, f.fy, f.lin, f.ang, pv);
  const float mag = sqrtf(pv[0] * pv[0] + pv[1] * pv[1]);
  *blur = f.E * mag;
  *skew = (f.T * mag) * fabsf(v / H - 0.5f);
  return pc[2] > clip && u >= 0.f && u < W && v >= 0.f && v < H;
}

// a visible pair joins the partial; an invisible one (whose values may be inf or nan) leaves it untouched
GS_HD void add_pair(Partial& a, bool visible, float blur, float skew) {
  const double b = visible ? (double)blur : 0.0;
  a.sum_blur += b;
  a.sum_sq += b * b;
  a.sum_skew += visible ? (double)skew : 0.0;
  a.max_blur = visible && blur > a.max_blur ? blur : a.max_blur;
  a.count += visible ? 1 : 0;
}

// stats[4] = mean_blur, rms_blur, max_blur, mean_skew
GS_HD void finish(const Partial& a, int* count, float stats[4]) {
  *count = a.count;
  if (a.count == 0) {
    stats[0] = stats[1] = stats[2] = stats[3] = 0.f;
    return;
  }
  const double n = (double)a.count;
  stats[0] = (float)(a.sum_blur / n);
  stats[1] = (float)::sqrt(a.sum_sq / n);
  stats[2] = a.max_blur;
  stats[3] = (float)(a.sum_skew / n);
}

}  // namespace blur
}  // namespace gs
