// TEST INFRASTRUCTURE ONLY: csrc/knn_math.h compiled for the host (tests/test_knn_host.py).  The cell rule, the hash, the
// shell walk with its stop rule and the top-k are the kernels'; the passes that the device runs as launches (bounds,
// sample, sort by bucket, bucket ranges, fallback list) run here row after row.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>
#include "knn_math.h"

namespace kn = gs::knn;

namespace {

template <int K>
void brute_row(int N, const float* xyz, int row, kn::TopK<K>& top) {
  top.clear();
  for (int j = 0; j < N; ++j) {
    if (j == row) continue;
    top.insert(kn::dist2(xyz[3 * row], xyz[3 * row + 1], xyz[3 * row + 2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]), j);
  }
}

template <int K>
void store_row(const kn::TopK<K>& top, int row, float* dists, int* idx) {
  for (int m = 0; m < K; ++m) {
    dists[(size_t)row * K + m] = kn::root(top.d2[m]);
    if (idx) idx[(size_t)row * K + m] = top.id[m];
  }
}

template <int K>
int run(int N, const float* xyz, float cell_size, int max_rings, int table_bits, float* dists, int* idx,
        int* stats) {
  float mn[3], mx[3], extent = 0.0f;
  for (int a = 0; a < 3; ++a) {
    mn[a] = mx[a] = xyz[a];
    for (int i = 1; i < N; ++i) { mn[a] = std::min(mn[a], xyz[3 * i + a]); mx[a] = std::max(mx[a], xyz[3 * i + a]); }
    extent = std::max(extent, mx[a] - mn[a]);
  }
  float h = cell_size;
  if (!(cell_size > 0.0f)) {
    const int S = kn::sample_count(N);
    std::vector<float> kth(S);
    for (int s = 0; s < S; ++s) {
      kn::TopK<K> top;
      brute_row<K>(N, xyz, kn::sample_row(N, s), top);
      kth[s] = kn::root(top.kth_d2());
    }
    std::sort(kth.begin(), kth.end());
    h = kn::auto_cell_size(kth[(S - 1) / 2], extent);
  }
  kn::Grid g;
  g.h = kn::clamp_cell_size(h, extent);
  for (int a = 0; a < 3; ++a) { g.mn[a] = mn[a]; g.gmax[a] = kn::cell_coord(mx[a], mn[a], g.h); }
  g.table_bits = table_bits > 0 ? table_bits : kn::table_bits_for(N);

  std::vector<unsigned> bucket(N);
  for (int i = 0; i < N; ++i) {
    int c[3];
    kn::point_cell(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], c);
    bucket[i] = kn::cell_bucket(c[0], c[1], c[2], g.table_bits);
  }
  std::vector<int> order(N);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bucket[a] < bucket[b]; });
  std::vector<kn::Point> pts(N);
  std::vector<unsigned long long> cells(N);
  std::vector<int> bins((size_t)2 << g.table_bits, 0);
  for (int s = 0; s < N; ++s) {
    const int i = order[s];
    pts[s].x = xyz[3 * i]; pts[s].y = xyz[3 * i + 1]; pts[s].z = xyz[3 * i + 2]; pts[s].idx = i;
    int c[3];
    kn::point_cell(g, pts[s].x, pts[s].y, pts[s].z, c);
    cells[s] = kn::cell_key(c[0], c[1], c[2]);
    const unsigned b = bucket[i];
    if (s == 0 || bucket[order[s - 1]] != b) bins[2 * b] = s;
    bins[2 * b + 1] = s + 1;
  }
  int fallback = 0;
  for (int s = 0; s < N; ++s) {
    kn::TopK<K> top;
    top.clear();
    const kn::Point q = pts[s];
    if (!kn::query_row<K>(g, max_rings, q.x, q.y, q.z, q.idx, bins.data(), pts.data(), cells.data(), top)) {
      ++fallback;
      brute_row<K>(N, xyz, q.idx, top);
    }
    store_row<K>(top, q.idx, dists, idx);
  }
  if (stats) {
    std::memcpy(&stats[0], &g.h, 4);
    stats[1] = max_rings; stats[2] = fallback; stats[3] = g.table_bits;
  }
  return 0;
}

}  // namespace

extern "C" {

int kh_cell_coord(float x, float mn, float h) { return kn::cell_coord(x, mn, h); }
float kh_stop_radius(int r, float h) { return kn::stop_radius(r, h); }
int kh_table_bits_for(int N) { return kn::table_bits_for(N); }
float kh_clamp_cell_size(float h, float extent) { return kn::clamp_cell_size(h, extent); }
unsigned kh_cell_bucket(int x, int y, int z, int bits) { return kn::cell_bucket(x, y, z, bits); }

// the whole search on the host, k a template parameter as in gs_knn; table_bits <= 0: the default
int kh_knn(int N, const float* xyz, int k, float cell_size, int max_rings, int table_bits, float* dists, int* idx,
           int* stats) {
  if (k < 1 || k > kn::kMaxK || N <= k) return 1;
  if (max_rings <= 0) max_rings = kn::kDefaultMaxRings;
  switch (k) {
#define KH_CASE(K) case K: return run<K>(N, xyz, cell_size, max_rings, table_bits, dists, idx, stats)
    KH_CASE(1); KH_CASE(2); KH_CASE(3); KH_CASE(4); KH_CASE(5); KH_CASE(6); KH_CASE(7); KH_CASE(8);
    KH_CASE(9); KH_CASE(10); KH_CASE(11); KH_CASE(12); KH_CASE(13); KH_CASE(14); KH_CASE(15); KH_CASE(16);
#undef KH_CASE
  }
  return 1;
}

}  // extern "C"
