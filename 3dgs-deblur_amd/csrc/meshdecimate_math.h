// meshdecimate_math.h — mesh decimation by vertex clustering with a quadric representative (meshdecimate.py).  Shared by
// csrc/meshdecimate.hip and the host build of tests/host_math/meshdecimate_host.cpp (TEST INFRASTRUCTURE ONLY; same
// arrangement as meshclean_math.h).  Both are compiled with -ffp-contract=off: every operation below rounds once, in the
// order written, so the two builds give the same bits.
//
// CELL      c = floor((double)v / s) per axis; the grid is anchored at the world origin.  A coordinate that is not finite,
//           or |c| > 2^30, is refused (kStatusBadVertex); a face index outside [0, V) is refused (kStatusBadFace) before it
//           is used as an index.
// CLUSTERS  the distinct cells, in ascending (cz, cy, cx); the members of a cluster in ascending vertex index.
// REPRESENTATIVE  in float64, relative to the cell centre o = (c + 0.5) s:
//   m        the mean of the members (sum in ascending vertex index, then one division per coordinate)
//   A, b     for every face in ascending index and each of its corners 0, 1, 2 that lies in the cluster (a face with two
//            corners here counts twice), with the corners p0, p1, p2 relative to o: n = (p1 - p0) x (p2 - p0), d = -n.p0,
//            A += n n^T, b += d n  (Lindstrom's area^2-weighted plane quadrics; faces that degenerate later still count)
//   y        lambda = 1e-3 tr(A); tr(A) zero or not finite: y = 0; otherwise (A + lambda I) y = -(b + A m) by the
//            square-root-free Cholesky factorisation L D L^T written out in solve() (only + - * / are used, each of which
//            rounds the same on both builds)
//   x        clamp(m + y, -s/2, s/2) per coordinate; the vertex is float32(o + x)
//   colour   the float64 mean of the members' colours, rounded to float32
// FACES     a face maps to the clusters of its corners; it is dropped (degenerate) when two of them coincide.  With
//           dedupe, of the faces with the same UNORDERED cluster triple only the one with the smallest index survives.
//           Survivors keep their corner order and their relative order.  A cluster that no surviving face refers to gives
//           no vertex; the output vertices are the referenced clusters in cluster order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_MD_HD __host__ __device__ __forceinline__
#else
#define GS_MD_HD inline
#endif

namespace gs {
namespace meshdecimate {

// the words of `counts` (device, kCountWords ints) that plan fills and the caller reads back once
constexpr int kCountWords = 8;
constexpr int kVertsOut = 0, kFacesOut = 1, kClusters = 2, kDegenerate = 3, kDuplicates = 4, kStatus = 5;
constexpr int kStatusBadFace = 1;      // a face index outside [0, V)
constexpr int kStatusBadVertex = 2;    // a coordinate that is not finite, or a cell index beyond +-2^30
constexpr int kMaxVerts = 1 << 30;
constexpr int kMaxFaces = 0x7fffffff / 3;      // 3 F fits an int: corner positions and the corner sort's payload
constexpr int kCellLimit = 1 << 30;
constexpr int kCellBias = 1 << 30;     // c + kCellBias is in [0, 2^31]: an unsigned 32-bit sort digit per axis

GS_MD_HD bool index_ok(int i, int V) { return (unsigned)i < (unsigned)V; }
GS_MD_HD bool face_ok(int a, int b, int c, int V) { return index_ok(a, V) && index_ok(b, V) && index_ok(c, V); }

// floor(x) for |x| <= 2^30 + 1, without the math library: the same instructions on both builds
GS_MD_HD double floor_small(double x) {
  const double t = (double)(long long)x;      // truncation towards zero
  return t > x ? t - 1.0 : t;
}

// the cell index of one coordinate -> false when it is refused (*c is then 0)
GS_MD_HD bool cell_of(float v, double s, int* c) {
  const double q = (double)v / s;
  *c = 0;
  if (!(q >= -(double)kCellLimit - 1.0 && q <= (double)kCellLimit + 1.0)) return false;      // NaN and infinities too
  const double f = floor_small(q);
  if (f < -(double)kCellLimit || f > (double)kCellLimit) return false;
  *c = (int)f;
  return true;
}

GS_MD_HD unsigned cell_digit(int c) { return (unsigned)(c + kCellBias); }
// the 64-bit major key of a cell: z above y (x is sorted first, in a 32-bit pass of its own)
GS_MD_HD unsigned long long cell_key_zy(int cy, int cz) {
  return ((unsigned long long)cell_digit(cz) << 32) | (unsigned long long)cell_digit(cy);
}

GS_MD_HD double cell_centre(int c, double s) { return ((double)c + 0.5) * s; }

// the sums of one cluster
struct Cluster {
  double o[3];                       // cell centre
  double sum[3], csum[3];            // members relative to o; their colours
  long long members;
  double a00, a01, a02, a11, a12, a22, b0, b1, b2;
};

GS_MD_HD void cluster_begin(Cluster* q, int cx, int cy, int cz, double s) {
  q->o[0] = cell_centre(cx, s); q->o[1] = cell_centre(cy, s); q->o[2] = cell_centre(cz, s);
  for (int k = 0; k < 3; ++k) { q->sum[k] = 0.0; q->csum[k] = 0.0; }
  q->members = 0;
  q->a00 = q->a01 = q->a02 = q->a11 = q->a12 = q->a22 = 0.0;
  q->b0 = q->b1 = q->b2 = 0.0;
}

// one member, in ascending vertex index; color may be null
GS_MD_HD void cluster_add_member(Cluster* q, const float* vert, const float* color) {
  for (int k = 0; k < 3; ++k) q->sum[k] = q->sum[k] + ((double)vert[k] - q->o[k]);
  if (color)
    for (int k = 0; k < 3; ++k) q->csum[k] = q->csum[k] + (double)color[k];
  q->members += 1;
}

// one (face, corner in this cluster), in ascending (face, corner); v0, v1, v2 are the face's corners 0, 1, 2
GS_MD_HD void cluster_add_face(Cluster* q, const float* v0, const float* v1, const float* v2) {
  double p0[3], e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    p0[k] = (double)v0[k] - q->o[k];
    const double p1 = (double)v1[k] - q->o[k], p2 = (double)v2[k] - q->o[k];
    e1[k] = p1 - p0[k];
    e2[k] = p2 - p0[k];
  }
  const double n0 = e1[1] * e2[2] - e1[2] * e2[1];
  const double n1 = e1[2] * e2[0] - e1[0] * e2[2];
  const double n2 = e1[0] * e2[1] - e1[1] * e2[0];
  const double d = -((n0 * p0[0] + n1 * p0[1]) + n2 * p0[2]);
  q->a00 = q->a00 + n0 * n0; q->a01 = q->a01 + n0 * n1; q->a02 = q->a02 + n0 * n2;
  q->a11 = q->a11 + n1 * n1; q->a12 = q->a12 + n1 * n2; q->a22 = q->a22 + n2 * n2;
  q->b0 = q->b0 + d * n0; q->b1 = q->b1 + d * n1; q->b2 = q->b2 + d * n2;
}

GS_MD_HD bool finite_d(double x) { return x - x == 0.0; }

// the representative as float32 world coordinates; color_out may be null
GS_MD_HD void cluster_solve(const Cluster* q, double s, float* vert_out, float* color_out) {
  const double count = (double)q->members;
  double m[3], y[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 3; ++k) m[k] = q->sum[k] / count;
  const double tr = (q->a00 + q->a11) + q->a22;
  if (finite_d(tr) && tr != 0.0) {
    const double lambda = 1e-3 * tr;
    const double m00 = q->a00 + lambda, m11 = q->a11 + lambda, m22 = q->a22 + lambda;
    const double m01 = q->a01, m02 = q->a02, m12 = q->a12;
    const double r0 = -(q->b0 + ((q->a00 * m[0] + q->a01 * m[1]) + q->a02 * m[2]));
    const double r1 = -(q->b1 + ((q->a01 * m[0] + q->a11 * m[1]) + q->a12 * m[2]));
    const double r2 = -(q->b2 + ((q->a02 * m[0] + q->a12 * m[1]) + q->a22 * m[2]));
    // M = L D L^T, L unit lower triangular
    const double d0 = m00;
    const double l10 = m01 / d0, l20 = m02 / d0;
    const double d1 = m11 - l10 * l10 * d0;
    const double l21 = (m12 - l20 * l10 * d0) / d1;
    const double d2 = m22 - (l20 * l20 * d0 + l21 * l21 * d1);
    // L z = r, D w = z, L^T y = w
    const double z0 = r0;
    const double z1 = r1 - l10 * z0;
    const double z2 = r2 - (l20 * z0 + l21 * z1);
    const double w0 = z0 / d0, w1 = z1 / d1, w2 = z2 / d2;
    y[2] = w2;
    y[1] = w1 - l21 * y[2];
    y[0] = w0 - (l10 * y[1] + l20 * y[2]);
    if (!(finite_d(y[0]) && finite_d(y[1]) && finite_d(y[2]))) y[0] = y[1] = y[2] = 0.0;
  }
  const double half = 0.5 * s;
  for (int k = 0; k < 3; ++k) {
    double x = m[k] + y[k];
    x = x < -half ? -half : (x > half ? half : x);
    vert_out[k] = (float)(q->o[k] + x);
  }
  if (color_out)
    for (int k = 0; k < 3; ++k) color_out[k] = (float)(q->csum[k] / count);
}

// the canonical (sorted) form of a cluster triple: lo <= mid <= hi
GS_MD_HD void sort3(int a, int b, int c, int* lo, int* mid, int* hi) {
  int t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
  *lo = a; *mid = b; *hi = c;
}

GS_MD_HD bool degenerate(int a, int b, int c) { return a == b || b == c || a == c; }

// the bits that hold every value of [0, n): at least 1
GS_MD_HD int index_bits(int n) {
  int bits = 1;
  while (bits < 31 && (1ll << bits) < (long long)n) ++bits;
  return bits;
}

}  // namespace meshdecimate
}  // namespace gs
