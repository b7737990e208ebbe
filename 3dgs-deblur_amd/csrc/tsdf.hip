// tsdf.hip — TSDF fusion of depth maps into a volume and marching-tetrahedra mesh extraction from it (tsdf.py).  The update
// rule, the tetrahedra, the triangle table and the orders: tsdf_math.h.  gfx950, wave64.
//
// INTEGRATE  one launch applies up to kFramesPerLaunch frames.  A workgroup is kBlockX x kBlockY voxels: one lane per voxel
//   along x (a wave moves 256 contiguous bytes per field), one wave per row.  The voxel's state is read once, kept in
//   registers across the frame loop and written once, and only if a frame touched it.  The camera of frame f (12 matrix
//   floats, 4 intrinsics) and the image base are the same for every lane, so they are read through uniform addresses
//   (scalar loads).  A voxel's result depends on its own index and the frames in order, nothing else.
// EXTRACT    count -> exclusive integer scan -> emit, no atomics, no workgroup waits on another:
//   1. count: one thread per sample: the 7-bit mask of its owned edges that carry a vertex and the faces of its cell, kept
//      as info[s]; every workgroup of kCountBlock samples stores its two totals;
//   2. scan of the workgroup totals, reduce-then-scan in three launches: totals per kScanBlock workgroups, one workgroup
//      that scans those (at most kMaxSuper of them) and stores V and F, then the prefix of every workgroup;
//   3. vertices: the workgroup's prefix plus a scan inside the workgroup gives every sample its first vertex index
//      (stored for the faces), the vertices are written;
//   4. faces: the same for the faces; a triangle finds the index of a vertex from its owner's first index and mask.
#include "gs_common.h"
#include "tsdf_math.h"

namespace {

namespace ts = gs::tsdf;

constexpr int kBlockX = 64, kBlockY = 4;          // integrate: voxels per workgroup
constexpr int kCountBlock = 256;                  // extraction: samples per workgroup
constexpr int kScanItems = 4;
constexpr int kScanBlock = 256 * kScanItems;      // workgroup totals per workgroup of the scan
constexpr int kMaxSuper = 4096;                   // 2^30 / kCountBlock / kScanBlock
constexpr int kTopItems = kMaxSuper / 256;

static_assert(kBlockX == gs::kWave, "one lane per voxel along x");
static_assert(ts::kMaxVoxels / kCountBlock / kScanBlock <= kMaxSuper, "three levels cover the largest volume");

__global__ __launch_bounds__(kBlockX * kBlockY) void tsdf_integrate_kernel(
    int nx, int ny, float ox, float oy, float oz, float voxel_size, float* __restrict__ tsdf, float* __restrict__ weight,
    float* __restrict__ color, int frames, int H, int W, const float* __restrict__ depth,
    const float* __restrict__ viewmats, const float* __restrict__ intrins, const float* __restrict__ cimg,
    const float* __restrict__ wimg, float trunc, float depth_min, float depth_max, float max_weight) {
  const int i = (int)(blockIdx.x * kBlockX + (threadIdx.x & (kBlockX - 1)));
  const int j = (int)(blockIdx.y * kBlockY + threadIdx.x / kBlockX);
  const int k = (int)blockIdx.z;
  if (i >= nx || j >= ny) return;
  const size_t s = ((size_t)k * ny + j) * nx + i;
  const float x = ts::sample_coord(ox, voxel_size, i), y = ts::sample_coord(oy, voxel_size, j),
              z = ts::sample_coord(oz, voxel_size, k);
  float f = tsdf[s], Wt = weight[s], cr = 0.0f, cg = 0.0f, cb = 0.0f;
  if (color) { cr = color[s * 3]; cg = color[s * 3 + 1]; cb = color[s * 3 + 2]; }
  bool touched = false;
  const size_t pixels = (size_t)H * W;
  for (int fr = 0; fr < frames; ++fr) {
    ts::Camera cam;
    ts::load_camera(viewmats + (size_t)fr * 16, intrins + (size_t)fr * 4, cam);      // uniform addresses
    float zc, val;
    int px, py;
    if (!ts::project(cam, x, y, z, W, H, &zc, &px, &py)) continue;
    const size_t p = (size_t)fr * pixels + (size_t)py * W + px;
    const float D = depth[p], w = wimg ? wimg[p] : 1.0f;
    if (!ts::depth_sample(D, w, zc, trunc, depth_min, depth_max, &val)) continue;
    const float Wn = Wt + w;
    f = ts::blend(f, Wt, val, w, Wn);
    if (color) {
      cr = ts::blend(cr, Wt, cimg[p * 3], w, Wn);
      cg = ts::blend(cg, Wt, cimg[p * 3 + 1], w, Wn);
      cb = ts::blend(cb, Wt, cimg[p * 3 + 2], w, Wn);
    }
    Wt = fminf(Wn, max_weight);
    touched = true;
  }
  if (touched) {
    tsdf[s] = f; weight[s] = Wt;
    if (color) { color[s * 3] = cr; color[s * 3 + 1] = cg; color[s * 3 + 2] = cb; }
  }
}

// ---- extraction ---------------------------------------------------------------------------------------------------------
// exclusive scan of one value per thread over a workgroup of 256; *total: the workgroup's sum (every thread)
__device__ __forceinline__ unsigned long long block_scan(unsigned long long v, unsigned long long* wave_tot,
                                                         unsigned long long* total) {
  const int lane = gs::lane_id(), wave = (int)threadIdx.x / gs::kWave;
  unsigned long long inc = v;
#pragma unroll
  for (int o = 1; o < gs::kWave; o <<= 1) {
    const unsigned long long up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  __syncthreads();                                  // wave_tot may still be read from an earlier call
  if (lane == gs::kWave - 1) wave_tot[wave] = inc;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned long long t = wave_tot[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

__device__ __forceinline__ void sample_ijk(const ts::Grid& g, size_t s, int* i, int* j, int* k) {
  *i = (int)(s % (size_t)g.nx);
  const size_t r = s / (size_t)g.nx;
  *j = (int)(r % (size_t)g.ny);
  *k = (int)(r / (size_t)g.ny);
}

// info[s] = edge mask | faces << 8; blk[b] = vertices | faces << 16 of workgroup b
__global__ __launch_bounds__(kCountBlock) void tsdf_count_kernel(ts::Grid g, long long n, const float* __restrict__ tsdf,
                                                                  const float* __restrict__ weight,
                                                                  unsigned short* __restrict__ info,
                                                                  unsigned* __restrict__ blk) {
  __shared__ unsigned long long wave_tot[4];
  const size_t s = (size_t)blockIdx.x * kCountBlock + threadIdx.x;
  unsigned v = 0, f = 0;
  if (s < (size_t)n) {
    int i, j, k;
    sample_ijk(g, s, &i, &j, &k);
    const int em = ts::sample_edges(g, tsdf, weight, i, j, k);
    f = (unsigned)ts::cell_faces(g, tsdf, weight, i, j, k);
    v = (unsigned)ts::popcount7(em);
    info[s] = (unsigned short)(em | (f << 8));
  }
  unsigned long long total;
  block_scan((unsigned long long)(v | (f << 16)), wave_tot, &total);
  if (threadIdx.x == 0) blk[blockIdx.x] = (unsigned)total;
}

// totals of kScanBlock workgroups: super_v[sb], super_f[sb]
__global__ __launch_bounds__(256) void tsdf_scan_reduce_kernel(long long nb, const unsigned* __restrict__ blk,
                                                                unsigned long long* __restrict__ super_v,
                                                                unsigned long long* __restrict__ super_f) {
  __shared__ unsigned long long wave_tot[4];
  unsigned long long v = 0, f = 0;
  for (int q = 0; q < kScanItems; ++q) {
    const long long b = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems + q;
    if (b < nb) { const unsigned t = blk[b]; v += t & 0xffffu; f += t >> 16; }
  }
  unsigned long long tv, tf;
  block_scan(v, wave_tot, &tv);
  block_scan(f, wave_tot, &tf);
  if (threadIdx.x == 0) { super_v[blockIdx.x] = tv; super_f[blockIdx.x] = tf; }
}

// one workgroup: exclusive scan of the at most kMaxSuper totals in place, and V, F (-1: more than an int holds)
__global__ __launch_bounds__(256) void tsdf_scan_top_kernel(int ns, unsigned long long* __restrict__ super_v,
                                                             unsigned long long* __restrict__ super_f,
                                                             int* __restrict__ counts) {
  __shared__ unsigned long long wave_tot[4];
  const int t = (int)threadIdx.x;
  unsigned long long v[kTopItems], f[kTopItems], sv = 0, sf = 0;
#pragma unroll
  for (int q = 0; q < kTopItems; ++q) {
    const int e = t * kTopItems + q;
    v[q] = e < ns ? super_v[e] : 0ull; f[q] = e < ns ? super_f[e] : 0ull;
    sv += v[q]; sf += f[q];
  }
  unsigned long long tv, tf;
  unsigned long long pv = block_scan(sv, wave_tot, &tv);
  unsigned long long pf = block_scan(sf, wave_tot, &tf);
#pragma unroll
  for (int q = 0; q < kTopItems; ++q) {
    const int e = t * kTopItems + q;
    if (e < ns) { super_v[e] = pv; super_f[e] = pf; }
    pv += v[q]; pf += f[q];
  }
  if (t == 0) {
    counts[0] = tv <= 0x7fffffffull ? (int)tv : -1;
    counts[1] = tf <= 0x7fffffffull ? (int)tf : -1;
  }
}

// prefix of every workgroup of the count: blk_v[b], blk_f[b]
__global__ __launch_bounds__(256) void tsdf_scan_apply_kernel(long long nb, const unsigned* __restrict__ blk,
                                                               const unsigned long long* __restrict__ super_v,
                                                               const unsigned long long* __restrict__ super_f,
                                                               unsigned* __restrict__ blk_v, unsigned* __restrict__ blk_f) {
  __shared__ unsigned long long wave_tot[4];
  unsigned v[kScanItems], f[kScanItems];
  unsigned long long sv = 0, sf = 0;
  const long long b0 = (long long)blockIdx.x * kScanBlock + (long long)threadIdx.x * kScanItems;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    const unsigned t = b0 + q < nb ? blk[b0 + q] : 0u;
    v[q] = t & 0xffffu; f[q] = t >> 16;
    sv += v[q]; sf += f[q];
  }
  unsigned long long total;
  unsigned long long pv = block_scan(sv, wave_tot, &total) + super_v[blockIdx.x];
  unsigned long long pf = block_scan(sf, wave_tot, &total) + super_f[blockIdx.x];
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    if (b0 + q < nb) { blk_v[b0 + q] = (unsigned)pv; blk_f[b0 + q] = (unsigned)pf; }
    pv += v[q]; pf += f[q];
  }
}

__global__ __launch_bounds__(kCountBlock) void tsdf_verts_kernel(ts::Grid g, long long n, float ox, float oy, float oz,
                                                                  float voxel_size, const float* __restrict__ tsdf,
                                                                  const float* __restrict__ color,
                                                                  const unsigned short* __restrict__ info,
                                                                  const unsigned* __restrict__ blk_v,
                                                                  unsigned* __restrict__ first_vert, int V,
                                                                  float* __restrict__ verts, float* __restrict__ colors) {
  __shared__ unsigned long long wave_tot[4];
  const size_t s = (size_t)blockIdx.x * kCountBlock + threadIdx.x;
  const int em = s < (size_t)n ? (info[s] & 0x7f) : 0;
  unsigned long long total;
  unsigned at = blk_v[blockIdx.x] + (unsigned)block_scan((unsigned long long)ts::popcount7(em), wave_tot, &total);
  if (s >= (size_t)n) return;
  first_vert[s] = at;
  if (!em) return;
  int i, j, k;
  sample_ijk(g, s, &i, &j, &k);
  const float origin[3] = {ox, oy, oz};
  for (int type = 0; type < ts::kEdgeTypes; ++type) {
    if (!((em >> type) & 1)) continue;
    float p[3], c[3];
    ts::edge_vertex(g, tsdf, colors ? color : nullptr, origin, voxel_size, i, j, k, type, p, c);
    if (at < (unsigned)V) {
      verts[(size_t)at * 3] = p[0]; verts[(size_t)at * 3 + 1] = p[1]; verts[(size_t)at * 3 + 2] = p[2];
      if (colors) { colors[(size_t)at * 3] = c[0]; colors[(size_t)at * 3 + 1] = c[1]; colors[(size_t)at * 3 + 2] = c[2]; }
    }
    ++at;
  }
}

__global__ __launch_bounds__(kCountBlock) void tsdf_faces_kernel(ts::Grid g, long long n, const float* __restrict__ tsdf,
                                                                  const unsigned short* __restrict__ info,
                                                                  const unsigned* __restrict__ blk_f,
                                                                  const unsigned* __restrict__ first_vert, int F,
                                                                  int* __restrict__ faces) {
  __shared__ unsigned long long wave_tot[4];
  const size_t s = (size_t)blockIdx.x * kCountBlock + threadIdx.x;
  const int nf = s < (size_t)n ? (info[s] >> 8) : 0;
  unsigned long long total;
  unsigned at = blk_f[blockIdx.x] + (unsigned)block_scan((unsigned long long)nf, wave_tot, &total);
  if (!nf) return;
  int i, j, k;
  sample_ijk(g, s, &i, &j, &k);
  const int cm = ts::cell_mask(g, tsdf, i, j, k);
  for (int tet = 0; tet < 6; ++tet) {
    const int m = ts::tet_case(cm, tet), nt = ts::case_triangles(m);
    for (int tri = 0; tri < nt; ++tri) {
      int ea[3], eb[3], idx[3];
      ts::case_triangle(m, ts::tet_odd(tet), tri, ea, eb);
      for (int e = 0; e < 3; ++e) {
        const int ca = ts::tet_corner(tet, ea[e]), cb = ts::tet_corner(tet, eb[e]);
        const size_t owner = ts::linear(g, i + (ca & 1), j + ((ca >> 1) & 1), k + (ca >> 2));
        const int type = ts::edge_type_of_code(ca ^ cb);
        idx[e] = (int)(first_vert[owner] + (unsigned)ts::popcount7(info[owner] & ((1 << type) - 1)));
      }
      if (at < (unsigned)F) { faces[(size_t)at * 3] = idx[0]; faces[(size_t)at * 3 + 1] = idx[1]; faces[(size_t)at * 3 + 2] = idx[2]; }
      ++at;
    }
  }
}

long long align256(long long b) { return (b + 255) & ~255ll; }

struct Layout {
  long long n, nb, ns, info, first_vert, blk, blk_v, blk_f, super_v, super_f, total;
};

Layout layout(int nx, int ny, int nz) {
  Layout L;
  L.n = (long long)nx * ny * nz;
  L.nb = (L.n + kCountBlock - 1) / kCountBlock;
  L.ns = (L.nb + kScanBlock - 1) / kScanBlock;
  long long o = 0;
  auto take = [&o](long long bytes) { const long long at = o; o += align256(bytes); return at; };
  L.info = take(2 * L.n);
  L.first_vert = take(4 * L.n);
  L.blk = take(4 * L.nb); L.blk_v = take(4 * L.nb); L.blk_f = take(4 * L.nb);
  L.super_v = take(8 * L.ns); L.super_f = take(8 * L.ns);
  L.total = o;
  return L;
}

bool finite(float v) { return v == v && v <= 3.0e38f && v >= -3.0e38f; }

#define TSDF_LAUNCHED() do { const int status_ = gs_launch_status(); if (status_ != GS_OK) return status_; } while (0)

}  // namespace

// see include/gsdeblur.h
GS_EXPORT int gs_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float* tsdf,
                                float* weight, float* color, int B, int H, int W, const float* depth,
                                const float* viewmats, const float* intrins, const float* color_images,
                                const float* weight_images, float trunc, float depth_min, float depth_max,
                                float max_weight, void* stream) {
  if (!ts::dims_ok(nx, ny, nz) || B < 0 || H < 1 || W < 1 || H > ts::kMaxImageDim || W > ts::kMaxImageDim) return GS_ERR_INVALID;
  if (!finite(ox) || !finite(oy) || !finite(oz) || !finite(voxel_size) || !(voxel_size > 0.0f)) return GS_ERR_INVALID;
  if (!finite(trunc) || !(trunc > 0.0f) || !(max_weight > 0.0f)) return GS_ERR_INVALID;
  if (depth_min != depth_min || depth_max != depth_max) return GS_ERR_INVALID;
  if (!tsdf || !weight) return GS_ERR_INVALID;
  if ((color == nullptr) != (color_images == nullptr)) return GS_ERR_INVALID;
  if (B == 0) return GS_OK;
  if (!depth || !viewmats || !intrins) return GS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((nx + kBlockX - 1) / kBlockX), (unsigned)((ny + kBlockY - 1) / kBlockY), (unsigned)nz);
  const size_t pixels = (size_t)H * W;
  for (int b0 = 0; b0 < B; b0 += ts::kFramesPerLaunch) {
    const int frames = B - b0 < ts::kFramesPerLaunch ? B - b0 : ts::kFramesPerLaunch;
    hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(kBlockX * kBlockY), 0, st, nx, ny, ox, oy, oz, voxel_size, tsdf,
                       weight, color, frames, H, W, depth + (size_t)b0 * pixels, viewmats + (size_t)b0 * 16,
                       intrins + (size_t)b0 * 4, color_images ? color_images + (size_t)b0 * pixels * 3 : nullptr,
                       weight_images ? weight_images + (size_t)b0 * pixels : nullptr, trunc, depth_min, depth_max,
                       max_weight);
    TSDF_LAUNCHED();
  }
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT long long gs_tsdf_mesh_workspace_bytes(int nx, int ny, int nz) {
  if (!ts::dims_ok(nx, ny, nz)) return -1;
  return layout(nx, ny, nz).total;
}

// see include/gsdeblur.h
GS_EXPORT int gs_tsdf_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float level,
                                 float min_weight, int* counts, void* ws, long long ws_bytes, void* stream) {
  if (!ts::dims_ok(nx, ny, nz) || !tsdf || !weight || !counts || !ws || ((uintptr_t)ws & 255)) return GS_ERR_INVALID;
  if (level != level || min_weight != min_weight) return GS_ERR_INVALID;
  const Layout L = layout(nx, ny, nz);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  char* w = reinterpret_cast<char*>(ws);
  hipStream_t st = (hipStream_t)stream;
  const ts::Grid g = {nx, ny, nz, level, min_weight};
  unsigned* blk = reinterpret_cast<unsigned*>(w + L.blk);
  unsigned long long* super_v = reinterpret_cast<unsigned long long*>(w + L.super_v);
  unsigned long long* super_f = reinterpret_cast<unsigned long long*>(w + L.super_f);
  hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)L.nb), dim3(kCountBlock), 0, st, g, L.n, tsdf, weight,
                     reinterpret_cast<unsigned short*>(w + L.info), blk);
  TSDF_LAUNCHED();
  hipLaunchKernelGGL(tsdf_scan_reduce_kernel, dim3((unsigned)L.ns), dim3(256), 0, st, L.nb, blk, super_v, super_f);
  TSDF_LAUNCHED();
  hipLaunchKernelGGL(tsdf_scan_top_kernel, dim3(1), dim3(256), 0, st, (int)L.ns, super_v, super_f, counts);
  TSDF_LAUNCHED();
  hipLaunchKernelGGL(tsdf_scan_apply_kernel, dim3((unsigned)L.ns), dim3(256), 0, st, L.nb, blk, super_v, super_f,
                     reinterpret_cast<unsigned*>(w + L.blk_v), reinterpret_cast<unsigned*>(w + L.blk_f));
  TSDF_LAUNCHED();
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT int gs_tsdf_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf,
                                const float* color, float level, int V, int F, float* verts, int* faces, float* colors,
                                void* ws, long long ws_bytes, void* stream) {
  if (!ts::dims_ok(nx, ny, nz) || V < 0 || F < 0 || !tsdf || !ws || ((uintptr_t)ws & 255)) return GS_ERR_INVALID;
  if (level != level || !finite(ox) || !finite(oy) || !finite(oz) || !finite(voxel_size)) return GS_ERR_INVALID;
  if (colors && !color) return GS_ERR_INVALID;
  const Layout L = layout(nx, ny, nz);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  if (V == 0 && F == 0) return GS_OK;
  if (!verts || !faces) return GS_ERR_INVALID;
  char* w = reinterpret_cast<char*>(ws);
  hipStream_t st = (hipStream_t)stream;
  const ts::Grid g = {nx, ny, nz, level, 0.0f};            // the used cells are in info already
  const unsigned short* info = reinterpret_cast<const unsigned short*>(w + L.info);
  unsigned* first_vert = reinterpret_cast<unsigned*>(w + L.first_vert);
  hipLaunchKernelGGL(tsdf_verts_kernel, dim3((unsigned)L.nb), dim3(kCountBlock), 0, st, g, L.n, ox, oy, oz, voxel_size, tsdf,
                     color, info, reinterpret_cast<const unsigned*>(w + L.blk_v), first_vert, V, verts, colors);
  TSDF_LAUNCHED();
  hipLaunchKernelGGL(tsdf_faces_kernel, dim3((unsigned)L.nb), dim3(kCountBlock), 0, st, g, L.n, tsdf, info,
                     reinterpret_cast<const unsigned*>(w + L.blk_f), first_vert, F, faces);
  TSDF_LAUNCHED();
  return GS_OK;
}
