// knn.hip — exact k nearest neighbours of a point cloud against itself on a hashed uniform grid (knn.py: the scales of a
// model started from a seed cloud).  Math, the exactness argument and the shell walk: knn_math.h.  gfx950, wave64.
//
// One call, nothing read back:
//   1. bounds: the bounding box, through integer min / max atomics on order-preserving bit patterns;
//   2. sample (cell size not given): knn_brute_kernel finds the k-th neighbour distance of <= 1024 fixed-stride rows;
//   3. grid: one workgroup sorts the samples, takes the median and writes the Grid (cell size, origin, extent in cells);
//   4. cells: bucket of every row; gs_radix_sort_pairs_u32 sorts the rows by bucket; gather lays the rows (x, y, z, row)
//      and their packed cells out in that order; gs_tile_bin_edges_u32 gives every bucket its range;
//   5. query: one thread per row in bucket order (the lanes of a wave share cells, so their bucket walks mostly read the
//      same lines), top-k in registers, rows still open after max_rings shells go to a list (integer atomic counter);
//   6. fallback: knn_brute_kernel resolves the listed rows, one workgroup per row: every thread keeps the top-k of its
//      stride of the cloud, the 256 lists are merged pairwise in LDS by (d2, index).
// No float atomics.  The list's order varies between runs; what is written for a row does not: the k best pairs under a
// total order, whichever kernel finds them.
#include "gs_common.h"
#include "knn_math.h"

namespace {

namespace kn = gs::knn;

constexpr int kThreads = 256;
constexpr int kQueryBlock = 256;                  // rows per workgroup of the query kernel
constexpr int kBruteThreads = 256;
constexpr int kMaxFallbackGroups = 2048;          // workgroups that share the fallback list: eight per CU
constexpr int kBoundsGroups = 1024;

// workspace header (device): the Grid, then the bounding box as order-preserving bit patterns and the fallback counter
struct Header {
  kn::Grid grid;
  unsigned lo[3], hi[3];
  unsigned fallback;
  unsigned pad;
};
static_assert(sizeof(Header) <= 256, "header");

__device__ __forceinline__ unsigned ordered_bits(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ void knn_init_kernel(Header* hd) {
  const int t = (int)threadIdx.x;
  if (t < 3) { hd->lo[t] = 0xffffffffu; hd->hi[t] = 0u; }
  if (t == 3) hd->fallback = 0u;
}

__global__ __launch_bounds__(kThreads) void knn_bounds_kernel(int N, const float* __restrict__ xyz, Header* hd) {
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int i = (int)(blockIdx.x * kThreads + threadIdx.x); i < N; i += (int)(gridDim.x * kThreads)) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned o = ordered_bits(xyz[(size_t)i * 3 + a]);
      lo[a] = min(lo[a], o); hi[a] = max(hi[a], o);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o));
      hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o));
    }
    if (gs::lane_id() == 0) { atomicMin(&hd->lo[a], lo[a]); atomicMax(&hd->hi[a], hi[a]); }
  }
}

// One workgroup per row, brute force over all N.  sample_out != NULL: the rows are the fixed-stride sample and only the
// k-th distance of each is kept; otherwise the rows are the fallback list and the full answer is written.  Workgroup 0
// of the fallback launch also writes the stats.
template <int K>
__global__ __launch_bounds__(kBruteThreads) void knn_brute_kernel(int N, const float* __restrict__ xyz,
                                                                   float* __restrict__ sample_out,
                                                                   const Header* __restrict__ hd,
                                                                   const int* __restrict__ list, int max_rings,
                                                                   float* __restrict__ dists, int* __restrict__ idx,
                                                                   int* __restrict__ stats) {
  __shared__ float s_d2[K * kBruteThreads];       // [entry][thread]: consecutive threads, consecutive banks
  __shared__ int s_id[K * kBruteThreads];
  const int t = (int)threadIdx.x;
  const int rows = sample_out ? kn::sample_count(N) : (int)hd->fallback;
  if (!sample_out && stats && blockIdx.x == 0 && t == 0) {
    stats[0] = __float_as_int(hd->grid.h); stats[1] = max_rings; stats[2] = rows; stats[3] = hd->grid.table_bits;
  }
  for (int f = (int)blockIdx.x; f < rows; f += (int)gridDim.x) {      // uniform per workgroup
    const int row = sample_out ? kn::sample_row(N, f) : list[f];
    const float qx = xyz[(size_t)row * 3], qy = xyz[(size_t)row * 3 + 1], qz = xyz[(size_t)row * 3 + 2];
    kn::TopK<K> top;
    top.clear();
    for (int j = t; j < N; j += kBruteThreads) {
      if (j == row) continue;
      top.insert(kn::dist2(qx, qy, qz, xyz[(size_t)j * 3], xyz[(size_t)j * 3 + 1], xyz[(size_t)j * 3 + 2]), j);
    }
    for (int s = kBruteThreads / 2; s >= 1; s >>= 1) {
      if (t >= s && t < 2 * s) {
#pragma unroll
        for (int m = 0; m < K; ++m) { s_d2[m * kBruteThreads + t] = top.d2[m]; s_id[m * kBruteThreads + t] = top.id[m]; }
      }
      __syncthreads();
      if (t < s) {
#pragma unroll
        for (int m = 0; m < K; ++m) top.insert(s_d2[m * kBruteThreads + t + s], s_id[m * kBruteThreads + t + s]);
      }
      __syncthreads();
    }
    if (t == 0) {
      if (sample_out) {
        sample_out[f] = kn::root(top.kth_d2());
      } else {
#pragma unroll
        for (int m = 0; m < K; ++m) {
          dists[(size_t)row * K + m] = kn::root(top.d2[m]);
          if (idx) idx[(size_t)row * K + m] = top.id[m];
        }
      }
    }
  }
}

// one workgroup of kSampleMax threads: bitonic sort of the sampled k-th distances, then the Grid
__global__ __launch_bounds__(kn::kSampleMax) void knn_grid_kernel(int N, float cell_size, const float* __restrict__ sample,
                                                                    Header* hd) {
  __shared__ float v[kn::kSampleMax];
  const int t = (int)threadIdx.x;
  const int S = cell_size > 0.0f ? 0 : kn::sample_count(N);
  v[t] = t < S ? sample[t] : INFINITY;
  __syncthreads();
  if (S > 0) {
    for (int size = 2; size <= kn::kSampleMax; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        const int o = t ^ stride;
        if (o > t) {
          const bool up = (t & size) == 0;
          const float a = v[t], b = v[o];
          if ((a > b) == up) { v[t] = b; v[o] = a; }
        }
        __syncthreads();
      }
    }
  }
  if (t == 0) {
    float mn[3], mx[3], extent = 0.0f;
    for (int a = 0; a < 3; ++a) {
      mn[a] = from_ordered_bits(hd->lo[a]); mx[a] = from_ordered_bits(hd->hi[a]);
      extent = fmaxf(extent, mx[a] - mn[a]);
    }
    float h = S > 0 ? kn::auto_cell_size(v[(S - 1) / 2], extent) : cell_size;
    h = kn::clamp_cell_size(h, extent);
    kn::Grid g;
    g.h = h;
    for (int a = 0; a < 3; ++a) { g.mn[a] = mn[a]; g.gmax[a] = kn::cell_coord(mx[a], mn[a], h); }
    g.table_bits = kn::table_bits_for(N);
    hd->grid = g;
  }
}

__global__ __launch_bounds__(kThreads) void knn_cells_kernel(int N, const float* __restrict__ xyz,
                                                              const Header* __restrict__ hd, unsigned* __restrict__ keys) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (i >= N) return;
  const kn::Grid g = hd->grid;
  int c[3];
  kn::point_cell(g, xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2], c);
  keys[i] = kn::cell_bucket(c[0], c[1], c[2], g.table_bits);
}

__global__ __launch_bounds__(kThreads) void knn_gather_kernel(int N, const float* __restrict__ xyz,
                                                               const Header* __restrict__ hd,
                                                               const unsigned* __restrict__ sorted_rows,
                                                               kn::Point* __restrict__ pts,
                                                               unsigned long long* __restrict__ cells) {
  const int s = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (s >= N) return;
  const kn::Grid g = hd->grid;
  const int i = (int)sorted_rows[s];
  kn::Point p;
  p.x = xyz[(size_t)i * 3]; p.y = xyz[(size_t)i * 3 + 1]; p.z = xyz[(size_t)i * 3 + 2]; p.idx = i;
  int c[3];
  kn::point_cell(g, p.x, p.y, p.z, c);
  pts[s] = p;
  cells[s] = kn::cell_key(c[0], c[1], c[2]);
}

template <int K>
__global__ __launch_bounds__(kQueryBlock) void knn_query_kernel(int N, int max_rings, Header* hd,
                                                                 const int* __restrict__ bins,
                                                                 const kn::Point* __restrict__ pts,
                                                                 const unsigned long long* __restrict__ cells,
                                                                 float* __restrict__ dists, int* __restrict__ idx,
                                                                 int* __restrict__ list) {
  const int s = (int)(blockIdx.x * kQueryBlock + threadIdx.x);
  if (s >= N) return;
  const kn::Grid g = hd->grid;
  const kn::Point q = pts[s];
  kn::TopK<K> top;
  top.clear();
  if (!kn::query_row<K>(g, max_rings, q.x, q.y, q.z, q.idx, bins, pts, cells, top)) {
    list[atomicAdd(&hd->fallback, 1u)] = q.idx;
    return;
  }
#pragma unroll
  for (int m = 0; m < K; ++m) {
    dists[(size_t)q.idx * K + m] = kn::root(top.d2[m]);
    if (idx) idx[(size_t)q.idx * K + m] = top.id[m];
  }
}

long long align256(long long b) { return (b + 255) & ~255ll; }

struct Layout {
  long long header, sample, keys0, vals0, keys1, vals1, pts, cells, bins, list, sort, total, sort_bytes;
  int table_bits;
};

Layout layout(int N) {
  Layout L;
  L.table_bits = kn::table_bits_for(N);
  long long o = 0;
  auto take = [&o](long long bytes) { const long long at = o; o += align256(bytes); return at; };
  L.header = take(sizeof(Header));
  L.sample = take(kn::kSampleMax * 4ll);
  L.keys0 = take(4ll * N); L.vals0 = take(4ll * N); L.keys1 = take(4ll * N); L.vals1 = take(4ll * N);
  L.pts = take(16ll * N);
  L.cells = take(8ll * N);
  L.bins = take(8ll << L.table_bits);
  L.list = take(4ll * N);
  L.sort_bytes = gs_radix_sort_workspace_bytes(N, 0, L.table_bits);
  L.sort = take(L.sort_bytes);
  L.total = o;
  return L;
}

bool shape_ok(int N, int k) { return k >= 1 && k <= kn::kMaxK && N > k && N <= kn::kMaxN; }

// K: the k of the call
template <int K>
int run(int N, const float* xyz, float cell_size, int max_rings, float* dists, int* idx, int* stats, char* ws,
        const Layout& L, hipStream_t st) {
  Header* hd = reinterpret_cast<Header*>(ws + L.header);
  float* sample = reinterpret_cast<float*>(ws + L.sample);
  unsigned* keys[2] = {reinterpret_cast<unsigned*>(ws + L.keys0), reinterpret_cast<unsigned*>(ws + L.keys1)};
  unsigned* vals[2] = {reinterpret_cast<unsigned*>(ws + L.vals0), reinterpret_cast<unsigned*>(ws + L.vals1)};
  kn::Point* pts = reinterpret_cast<kn::Point*>(ws + L.pts);
  unsigned long long* cells = reinterpret_cast<unsigned long long*>(ws + L.cells);
  int* bins = reinterpret_cast<int*>(ws + L.bins);
  int* list = reinterpret_cast<int*>(ws + L.list);
  const unsigned row_groups = (unsigned)((N + kThreads - 1) / kThreads);
  int status;
#define KNN_LAUNCHED() do { status = gs_launch_status(); if (status != GS_OK) return status; } while (0)
  hipLaunchKernelGGL(knn_init_kernel, dim3(1), dim3(64), 0, st, hd);
  KNN_LAUNCHED();
  hipLaunchKernelGGL(knn_bounds_kernel, dim3(row_groups < (unsigned)kBoundsGroups ? row_groups : (unsigned)kBoundsGroups),
                     dim3(kThreads), 0, st, N, xyz, hd);
  KNN_LAUNCHED();
  if (!(cell_size > 0.0f)) {
    hipLaunchKernelGGL((knn_brute_kernel<K>), dim3((unsigned)kn::sample_count(N)), dim3(kBruteThreads), 0, st, N, xyz,
                       sample, hd, nullptr, max_rings, nullptr, nullptr, nullptr);
    KNN_LAUNCHED();
  }
  hipLaunchKernelGGL(knn_grid_kernel, dim3(1), dim3(kn::kSampleMax), 0, st, N, cell_size > 0.0f ? cell_size : 0.0f, sample,
                     hd);
  KNN_LAUNCHED();
  hipLaunchKernelGGL(knn_cells_kernel, dim3(row_groups), dim3(kThreads), 0, st, N, xyz, hd, keys[0]);
  KNN_LAUNCHED();
  int buf = 0;
  status = gs_radix_sort_pairs_u32(N, keys[0], vals[0], keys[1], vals[1], 1, 0, L.table_bits, ws + L.sort, L.sort_bytes,
                                   &buf, st);
  if (status != GS_OK) return status;
  hipLaunchKernelGGL(knn_gather_kernel, dim3(row_groups), dim3(kThreads), 0, st, N, xyz, hd, vals[buf], pts, cells);
  KNN_LAUNCHED();
  status = gs_tile_bin_edges_u32(N, keys[buf], 1 << L.table_bits, bins, nullptr, st);
  if (status != GS_OK) return status;
  hipLaunchKernelGGL((knn_query_kernel<K>), dim3((unsigned)((N + kQueryBlock - 1) / kQueryBlock)), dim3(kQueryBlock), 0, st,
                     N, max_rings, hd, bins, pts, cells, dists, idx, list);
  KNN_LAUNCHED();
  hipLaunchKernelGGL((knn_brute_kernel<K>), dim3((unsigned)(N < kMaxFallbackGroups ? N : kMaxFallbackGroups)),
                     dim3(kBruteThreads), 0, st, N, xyz, nullptr, hd, list, max_rings, dists, idx, stats);
  KNN_LAUNCHED();
#undef KNN_LAUNCHED
  return GS_OK;
}

}  // namespace

// see include/gsdeblur.h
GS_EXPORT long long gs_knn_workspace_bytes(int N, int k) {
  if (!shape_ok(N, k)) return -1;
  return layout(N).total;
}

// see include/gsdeblur.h
GS_EXPORT int gs_knn(int N, const float* xyz, int k, float cell_size, int max_rings, float* dists, int* idx, int* stats,
                     void* ws, long long ws_bytes, void* stream) {
  if (!shape_ok(N, k) || !xyz || !dists || !ws || ((uintptr_t)ws & 255)) return GS_ERR_INVALID;
  if (cell_size != cell_size || cell_size > 3.0e38f) return GS_ERR_INVALID;
  const Layout L = layout(N);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  if (max_rings <= 0) max_rings = kn::kDefaultMaxRings;
  if (max_rings > 64) max_rings = 64;
  char* w = reinterpret_cast<char*>(ws);
  hipStream_t st = (hipStream_t)stream;
  switch (k) {
#define KNN_CASE(K) case K: return run<K>(N, xyz, cell_size, max_rings, dists, idx, stats, w, L, st)
    KNN_CASE(1); KNN_CASE(2); KNN_CASE(3); KNN_CASE(4); KNN_CASE(5); KNN_CASE(6); KNN_CASE(7); KNN_CASE(8);
    KNN_CASE(9); KNN_CASE(10); KNN_CASE(11); KNN_CASE(12); KNN_CASE(13); KNN_CASE(14); KNN_CASE(15); KNN_CASE(16);
#undef KNN_CASE
  }
  return GS_ERR_INVALID;
}
