// knn_math.h — the exact k-nearest-neighbour search of a point cloud against itself (knn.py: the scale of a Gaussian
// started from a seed cloud is the mean distance to its 3 nearest neighbours), shared by csrc/knn.hip and the host build
// of tests/host_math/knn_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as colorcorrect_math.h).
//
//   result   for row i the k smallest (squared distance, index) pairs over the rows j != i.  A row is excluded by index,
//            so a duplicate point is a neighbour at distance 0.  The order is total, so the k pairs do not depend on the
//            order in which candidates are met.  Returned distances are the square roots, ascending
//   distance d2 = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j, every operation rounded to float32 (no fused
//            multiply-add: both builds compile with -ffp-contract=off); the same bits from both sides of a pair
//   cell     h = 2 x (lower) median of the k-th neighbour distance of at most kSampleMax fixed-stride rows, each found by
//            brute force; h = extent / 64 (or 1 when the extent is 0 too) when that is 0; then h = max(h, extent / 2^21)
//            with extent the largest side of the bounding box.  A forced cell size gets the same clamp
//   grid     cell coordinate per axis c = clamp(floor((double(x) - double(min)) / double(h)), 0, 2^21 - 1); the three
//            coordinates pack into 63 bits; a cell hashes into a table of 2^table_bits >= 2N buckets; rows are sorted by
//            bucket, bins[b] = [begin, end) of bucket b in the sorted order
//   query    visit the Chebyshev shells r = 0 .. max_rings of the row's cell (cells outside [0, gmax] hold nothing and
//            are skipped).  A candidate of a bucket is accepted only when its own packed cell equals the visited cell:
//            two cells of one query can share a bucket, and each point is then met once, under its own cell.  After
//            shell r the row is done when the cube covers the whole grid, or when it holds k candidates and
//            root(d2_k) <= stop_radius(r, h), root() the correctly rounded float32 square root
//   exact    a row j outside the (2r+1)^3 cube differs from i by at least r + 1 cells on some axis, so the quotients
//            t = (x - min) / h differ by more than r there.  t is a double: its error is below 2^-30 cells for 21-bit
//            coordinates, so |x_i - x_j| > (r - 2^-29) h, and rounding the float32 subtraction, square, sums (of
//            non-negative terms) and root, all monotone, loses at most 3 x 2^-24 relatively: dist(i, j) > r h (1 - 2e-7).
//            stop_radius(r, h) = r h (1 - 2^-21), itself rounded twice, is at most r h (1 - 3.5e-7) and at least
//            r h (1 - 6.6e-7): strictly inside, so no such j can tie or beat the k-th candidate.  The clamp to 2^21 - 1 only
//            lowers coordinates, which can bring a cell nearer in the walk, never push it out
//   fallback a row still open after shell max_rings is resolved by brute force over all N (one workgroup per row)
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_KNN_HD __host__ __device__ __forceinline__
#else
#define GS_KNN_HD inline
#endif

namespace gs {
namespace knn {

constexpr int kMaxK = 16;
constexpr int kDefaultMaxRings = 8;
constexpr int kSampleMax = 1024;                 // rows whose k-th neighbour distance chooses the cell size
constexpr int kCoordBits = 21;
constexpr int kCoordMax = (1 << kCoordBits) - 1;
constexpr int kMaxN = 1 << 26;                   // the bucket table then has at most 2^27 entries
constexpr int kNoIndex = 0x7fffffff;

struct Grid {
  float mn[3];
  float h;
  int gmax[3];                                   // cell coordinates of the bounding box's maximum
  int table_bits;
};

struct alignas(16) Point {                       // a row in bucket-sorted order
  float x, y, z;
  int idx;                                       // its row in the input
};

GS_KNN_HD int table_bits_for(int N) {
  int b = 1;
  while ((1ll << b) < 2ll * N) ++b;
  return b;
}

GS_KNN_HD int sample_count(int N) { return N < kSampleMax ? N : kSampleMax; }
GS_KNN_HD int sample_row(int N, int s) { return s * (N / sample_count(N)); }

// median: the lower median of the sampled k-th distances; extent: the largest side of the bounding box
GS_KNN_HD float auto_cell_size(float median, float extent) {
  float h = 2.0f * median;
  if (!(h > 0.0f)) h = extent > 0.0f ? extent / 64.0f : 1.0f;
  return h;
}

GS_KNN_HD float clamp_cell_size(float h, float extent) {
  const float lo = extent / (float)(1 << kCoordBits);
  return h > lo ? h : lo;
}

GS_KNN_HD int cell_coord(float x, float mn, float h) {
  const double t = floor(((double)x - (double)mn) / (double)h);
  return t < 0.0 ? 0 : (t > (double)kCoordMax ? kCoordMax : (int)t);
}

GS_KNN_HD unsigned long long cell_key(int cx, int cy, int cz) {
  return ((unsigned long long)cz << (2 * kCoordBits)) | ((unsigned long long)cy << kCoordBits) | (unsigned long long)cx;
}

GS_KNN_HD unsigned cell_bucket(int cx, int cy, int cz, int table_bits) {
  const unsigned hsh = ((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u) ^ ((unsigned)cz * 83492791u);
  return (hsh ^ (hsh >> 15)) & ((1u << table_bits) - 1u);
}

GS_KNN_HD void point_cell(const Grid& g, float x, float y, float z, int c[3]) {
  c[0] = cell_coord(x, g.mn[0], g.h);
  c[1] = cell_coord(y, g.mn[1], g.h);
  c[2] = cell_coord(z, g.mn[2], g.h);
}

GS_KNN_HD float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// the correctly rounded float32 square root, whatever the compiler's float32 sqrt is: a double holds the root of a
// float32 to more than twice its precision, so rounding it again is the rounding of the exact root
GS_KNN_HD float root(float d2) { return (float)sqrt((double)d2); }

GS_KNN_HD float stop_radius(int r, float h) { return ((float)r * h) * (1.0f - 1.0f / (float)(1 << 21)); }

GS_KNN_HD bool closer(float d2a, int ia, float d2b, int ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// the K best (d2, index) pairs met so far, ascending; K is the k of the call (a template parameter), and every index is
// a compile-time constant after unrolling, so the arrays live in registers
template <int K>
struct TopK {
  float d2[K];
  int id[K];
  GS_KNN_HD void clear() {
#pragma unroll
    for (int m = 0; m < K; ++m) { d2[m] = INFINITY; id[m] = kNoIndex; }
  }
  GS_KNN_HD void insert(float d, int i) {
    if (!closer(d, i, d2[K - 1], id[K - 1])) return;
    d2[K - 1] = d; id[K - 1] = i;
#pragma unroll
    for (int m = K - 1; m > 0; --m) {
      if (closer(d2[m], id[m], d2[m - 1], id[m - 1])) {
        const float td = d2[m]; d2[m] = d2[m - 1]; d2[m - 1] = td;
        const int ti = id[m]; id[m] = id[m - 1]; id[m - 1] = ti;
      }
    }
  }
  GS_KNN_HD float kth_d2() const { return d2[K - 1]; }
  GS_KNN_HD bool full() const { return id[K - 1] != kNoIndex; }
};

// the shell walk of one row (position q, input row `self`): true when `top` holds the exact answer, false when the row
// is still open after shell max_rings.  bins: (begin, end) per bucket; pts / keys: rows and their packed cells in
// bucket-sorted order
template <int K>
GS_KNN_HD bool query_row(const Grid& g, int max_rings, float qx, float qy, float qz, int self, const int* bins,
                         const Point* pts, const unsigned long long* keys, TopK<K>& top) {
  int c[3];
  point_cell(g, qx, qy, qz, c);
  for (int r = 0; r <= max_rings; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int z = c[2] + dz;
      if (z < 0 || z > g.gmax[2]) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int y = c[1] + dy;
        if (y < 0 || y > g.gmax[1]) continue;
        const bool face = dz == -r || dz == r || dy == -r || dy == r;
        const int step = face ? 1 : 2 * r;         // inside the slab only the two end cells belong to shell r
        for (int dx = -r; dx <= r; dx += step) {
          const int x = c[0] + dx;
          if (x < 0 || x > g.gmax[0]) continue;
          const unsigned b = cell_bucket(x, y, z, g.table_bits);
          const unsigned long long want = cell_key(x, y, z);
          const int begin = bins[2 * b], end = bins[2 * b + 1];
          for (int s = begin; s < end; ++s) {
            if (keys[s] != want) continue;
            const Point p = pts[s];
            if (p.idx == self) continue;
            top.insert(dist2(qx, qy, qz, p.x, p.y, p.z), p.idx);
          }
        }
      }
    }
    bool all = true;
    for (int a = 0; a < 3; ++a) all = all && c[a] - r <= 0 && c[a] + r >= g.gmax[a];
    if (all) return true;
    if (top.full() && root(top.kth_d2()) <= stop_radius(r, g.h)) return true;
  }
  return false;
}

}  // namespace knn
}  // namespace gs
