// tilecull_math.h — the exact tile cull's ellipse test: which tiles of a Gaussian's bounding box can hold a pixel with
// alpha = o * exp(-sigma) >= 1/255.  Shared by csrc/binning.hip (the exact count and both emissions) and the host build
// of tests/host_math/tilecull_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as knn_math.h, blur_math.h and
// colorcorrect_math.h).
//
//   record   rec[0..5] = (gx, gy, a, b, c, o): the splat's centre in pixels, its conic and its opacity
//   sigma    (a u^2 + 2 b u v + c v^2) / 2 with (u, v) = pixel centre - (gx, gy); a pixel takes a contribution only when
//            sigma <= ln(255 o)
//   tau      ln(255 o) * 1.001 + 1e-3 (the conservative slack folded in), -1 when o <= 0 or ln(255 o) < 0: no tile is hit
//   det      a c - b b of the float32 values to within two ulps of the result (conic_det: two explicit fmas)
//   derive   ustar = largest |u| on the ellipse * 1.0001, vext = largest |v| * 1.0001, vstar = b ustar / c; a conic with
//            det <= 0, a <= 0 or c <= 0 is never culled (ustar = 3e38)
//   row_span the one interval [ul, ur] of u the ellipse covers inside the band of pixel-centre rows of tile row ty (rows
//            clipped to H - 0.5), widened by eps = 2e-3 + 2e-6 (|gx| + ustar).  SWEEP: the centre moves,
//            (gx, gy) + t (pvx, pvy), t in [st0 + tr(y), st1 + tr(y)], tr(y) = ((y + 0.5) / H - 0.5) srs; the band and the
//            interval are widened by the box of offsets the centre takes over the rows of the tile row, plus
//            1e-3 + 1e-5 (|t_lo| + |t_hi|) (|pvx| + |pvy|)
//   tiles    tile tx holds the pixel centres 16 tx + 0.5 .. 16 tx + 15.5 (the last column of the image keeps its full
//            width: conservative)
//
// Every function disables contraction (the count and the emissions must take the SAME decision for a tile wherever
// this is inlined); the host build compiles with -ffp-contract=off.  The logarithm is __logf on the device and logf on
// the host: the two builds can differ for a tile only through it.
#pragma once
#include <math.h>
#include "gs_math.h"

#if defined(__HIPCC__)
#define GS_TC_HD __host__ __device__ __forceinline__
#else
#define GS_TC_HD inline
#endif

namespace gs {

#if defined(__HIP_DEVICE_COMPILE__)
#define GS_TC_LOGF(x) __logf(x)
#else
#define GS_TC_LOGF(x) logf(x)
#endif

struct Ellipse { float gx, gy, a, b, c, tau, ra, rc, ustar, vstar, vext;
                 // swept form (round 6, pixel-velocity compositors): the centre moves, gx + t pvx, gy + t pvy, over the
                 // times the pixels of a tile row can see it: t in [st0 + tau(row), st1 + tau(row)], tau(y) = ((y + .5)/H - .5) srs
                 float pvx, pvy, st0, st1, srs; };
// ustar = largest |u| on the ellipse (reached at v = -b*ustar/c), vext = largest |v|, vstar = b*ustar/c

// The determinant the tile tests work with.  a c - b b in float32 is two rounded products: its absolute error is up to
// 2^-23 a c, which is ALL of the value for a needle (det / (a c) = 4 / anisotropy^2 at 45 degrees: below 2^-23 from an
// anisotropy of 6000).  A determinant that is noise but happens to come out positive gave extents that were too small,
// and tiles holding pixels with alpha >= 1/255 were culled (tests/test_slicefront_host.py: 10 of 3.8e7 fuzzed pairs).
// The tests therefore use the determinant of the float32 conic to within two ulps of its own value (Kahan's fused form:
// the rounding error of b b is recovered exactly by one fma and added back; the fmas are explicit, contraction stays
// off), which the 1.0001 on the extents covers with room to spare; when it is not positive the conic is degenerate and
// nothing is culled.  For a conic whose determinant was not noise the value moves by a few ulps.
GS_TC_HD float conic_det(float a, float b, float c) {
#pragma clang fp contract(off)
  const float w = b * b;
  const float e = fmaf(-b, b, w);                  // w - b b, exact
  const float f = fmaf(a, c, -w);                  // a c - w, one rounding
  return f + e;
}

// everything the tile tests need beyond (gx, gy, a, b, c, tau): the same arithmetic wherever an ellipse is rebuilt
// from those six numbers (LDS staging, v_readlane broadcast), so every copy takes identical decisions
GS_TC_HD void ellipse_derive(Ellipse& e) {
#pragma clang fp contract(off)
  e.ra = 1.0f / e.a; e.rc = 1.0f / e.c;
  // sigma = (a u^2 + 2 b u v + c v^2)/2 <= tau:  extent in u is sqrt(2 tau c / det), in v sqrt(2 tau a / det)
  const float det = conic_det(e.a, e.b, e.c);
  if (e.tau >= 0.f && det > 0.f && e.a > 0.f && e.c > 0.f) {
    const float k = 2.0f * e.tau / det;
    e.ustar = sqrtf(k * e.c) * 1.0001f;
    e.vext = sqrtf(k * e.a) * 1.0001f;
    e.vstar = e.b * e.ustar * e.rc;
  } else {
    e.ustar = e.vext = 3.0e38f;       // degenerate conic: never cull
    e.vstar = 0.f;
  }
}

GS_TC_HD Ellipse make_ellipse(const float* __restrict__ rec) {
#pragma clang fp contract(off)
  Ellipse e;
  e.gx = rec[0]; e.gy = rec[1]; e.a = rec[2]; e.b = rec[3]; e.c = rec[4];
  const float op = rec[5];
  e.tau = op > 0.f ? GS_TC_LOGF(255.0f * op) : -1.f;
  // threshold with the conservative slack folded in (the tile tests compare against it directly)
  e.tau = e.tau < 0.f ? -1.f : e.tau * 1.001f + 1e-3f;
  ellipse_derive(e);
  return e;
}

// Columns of pixel centres a tile ROW can reach.  The part of the ellipse inside the band v in [v0,v1] is convex,
// so its projection on u is ONE interval [ul, ur]: a tile of that row is hit iff its pixel-centre columns intersect
// it.  ur is the ellipse's overall extreme ustar when the line v = -vstar (where it is attained) crosses the band,
// else the larger of the two chord ends at the band edges; ul likewise with +vstar.  One evaluation per row (two
// square roots) instead of four edge minima per tile; exact up to rounding, which the slack (the enlarged tau plus
// an explicit margin on the interval) keeps on the conservative side.  Contraction is disabled: the count and the
// emission must take the SAME decision for every tile wherever this is inlined.
struct RowSpan { float ul, ur; };

template <bool SWEEP = false>
GS_TC_HD RowSpan row_span(const Ellipse& e, int ty, int H) {
#pragma clang fp contract(off)
  RowSpan r;
  r.ul = 1.f; r.ur = -1.f;                                 // empty
  if (e.tau < 0.f) return r;
  if (e.ustar > 1.0e37f) { r.ul = -3.0e38f; r.ur = 3.0e38f; return r; }
  float v0 = (float)(ty * K::kTile) + 0.5f - e.gy;
  float v1 = fminf((float)(ty * K::kTile + K::kTile) - 0.5f, (float)H - 0.5f) - e.gy;
  float ox0 = 0.f, ox1 = 0.f;
  if (SWEEP) {
    // SWEEP: the offsets the centre can have while a pixel of this tile row is exposed — x and y taken as independent
    // intervals (a box around the swept segment: conservative).  A pixel at (x, y) sees the splat at
    // (x - gx - ox, y - gy - oy): the row band widens by the y offsets, the column interval by the x offsets.
    const float invH = 1.0f / (float)H;
    const float ya = (float)(ty * K::kTile) + 0.5f, yb = fminf((float)(ty * K::kTile + K::kTile) - 0.5f, (float)H - 0.5f);
    const float ta = (ya * invH - 0.5f) * e.srs, tb = (yb * invH - 0.5f) * e.srs;
    const float t_lo = e.st0 + fminf(ta, tb), t_hi = e.st1 + fmaxf(ta, tb);
    const float slack = 1e-3f + 1e-5f * (fabsf(t_lo) + fabsf(t_hi)) * (fabsf(e.pvx) + fabsf(e.pvy));
    ox0 = fminf(t_lo * e.pvx, t_hi * e.pvx) - slack; ox1 = fmaxf(t_lo * e.pvx, t_hi * e.pvx) + slack;
    const float oy0 = fminf(t_lo * e.pvy, t_hi * e.pvy) - slack, oy1 = fmaxf(t_lo * e.pvy, t_hi * e.pvy) + slack;
    v0 -= oy1; v1 -= oy0;
  }
  if (v1 < -e.vext || v0 > e.vext) return r;
  const float w0 = fmaxf(v0, -e.vext), w1 = fminf(v1, e.vext);
  // chord of the ellipse on the line v = w: u = (-b w -/+ sqrt(2 a tau - det w^2)) / a
  const float det = conic_det(e.a, e.b, e.c);
  const float k2 = 2.0f * e.a * e.tau;
  const float d0 = sqrtf(fmaxf(k2 - det * w0 * w0, 0.f)), d1 = sqrtf(fmaxf(k2 - det * w1 * w1, 0.f));
  const float c0 = -e.b * w0, c1 = -e.b * w1;
  float ur = fmaxf((c0 + d0) * e.ra, (c1 + d1) * e.ra);
  float ul = fminf((c0 - d0) * e.ra, (c1 - d1) * e.ra);
  if (-e.vstar >= w0 && -e.vstar <= w1) ur = e.ustar;
  if (e.vstar >= w0 && e.vstar <= w1) ul = -e.ustar;
  const float eps = 2e-3f + 2e-6f * (fabsf(e.gx) + e.ustar);
  r.ur = fmaxf(ur, ul) + eps + ox1;
  r.ul = fminf(ul, ur) - eps + ox0;
  return r;
}

// first / one-past-last tile column of row ty whose pixel centres intersect the span, clamped to [x0, x1)
GS_TC_HD void span_tiles(const Ellipse& e, const RowSpan& sp, int x0, int x1, int& t0, int& t1) {
#pragma clang fp contract(off)
  if (sp.ur < sp.ul) { t0 = t1 = x0; return; }
  // tile tx holds pixel centres tx*16 + 0.5 .. tx*16 + 15.5 (the last column of the image may hold fewer: keeping
  // the full width there is conservative)
  const float lo = (sp.ul + e.gx - 15.5f) * (1.0f / (float)K::kTile);
  const float hi = (sp.ur + e.gx - 0.5f) * (1.0f / (float)K::kTile);
  const float flo = fminf(fmaxf(ceilf(lo), (float)x0), (float)x1);
  const float fhi = fminf(fmaxf(floorf(hi) + 1.0f, (float)x0), (float)x1);
  t0 = (int)flo; t1 = (int)fhi;
  if (t1 < t0) t1 = t0;
}

template <bool SWEEP = false>
GS_TC_HD bool tile_hit(const Ellipse& e, int tx, int ty, int W, int H) {
  (void)W;
  const RowSpan sp = row_span<SWEEP>(e, ty, H);
  int t0, t1;
  span_tiles(e, sp, tx, tx + 1, t0, t1);
  return t1 > t0;
}

}  // namespace gs
