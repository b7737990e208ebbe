// bilagrid.hip — bilateral-grid colour correction between the compositor and the loss (bilagrid.py): slice forward,
// slice backward (d loss / d rgb and the grid gradient) and the total-variation penalty.  Math: bilagrid_math.h.
// gfx950, wave64.
//
// A workgroup owns a tile of tw x th pixels (64 x 16 at training sizes; one wave per pixel row, lanes along x).  A tile
// touches few lattice vertices — at 1080p one cell of the 16 x 16 x 8 grid spans 128 x 72 pixels — so the tile's
// "footprint" (its vertex columns x its vertex rows x every L slice x 12 channels) is staged in LDS once and every pixel
// interpolates from there.
//
// The grid gradient is a sum of two million pixels into 24576 values.  It is formed without float atomics, in a fixed
// order, so that two runs agree bit for bit:
//   1. inside a wave (one pixel row) the lanes that share (x cell, L cell) are summed with the fixed DPP tree of
//      gs::wave_sum_uniform — 48 sums per group: {z0, z0+1} x {x0, x0+1} x 12; the row's y weights are uniform and are
//      applied afterwards — and lanes 0..47 add the results into the WAVE's own copy of the footprint in LDS;
//   2. the workgroup adds its four copies in wave order and stores ONE partial row (and its footprint) to the caller's
//      scratch;
//   3. bilagrid_reduce_kernel: one thread per grid value adds the partial rows that cover it, in (image, tile row, tile
//      column) order, and stores every value of v_grids, zeros included.
// Small frames put many cells under a tile: the host then picks a smaller tile (down to one pixel) so that the footprint
// still fits; correct for any H, W >= 1.
#include "gs_common.h"
#include "bilagrid_math.h"

namespace {

namespace bg = gs::bilagrid;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLdsBytes = 48 * 1024;

struct TilePlan {
  int tw, th;          // pixels per tile (tw <= 64 lanes, th rows dealt to the 4 waves)
  int ntx, nty;        // tiles per image
  int rowcap;          // floats of the largest footprint a tile of this size can have
};

// most vertices T consecutive pixels of an axis of `size` pixels can touch on an axis of n vertices: the positions of the
// first and the last pixel differ by (T-1)(n-1)/size, which touches at most floor(.) + 2 vertices; + 1 covers the
// rounding of the float positions
int foot_bound(int T, int n, int size) {
  if (T > size) T = size;
  const long long b = ((long long)(T - 1) * (long long)(n - 1)) / (long long)size + 3;
  return b < n ? (int)b : n;
}

// the largest tile whose footprint (copies: 1 for the staged grid, + kWaves accumulators in the backward) fits in LDS
bool make_plan(int H, int W, int GW, int GH, int L, int copies, TilePlan& p) {
  const int cand[6][2] = {{64, 16}, {64, 4}, {16, 4}, {4, 4}, {2, 2}, {1, 1}};
  for (const auto& c : cand) {
    const long long cap = (long long)foot_bound(c[0], GW, W) * foot_bound(c[1], GH, H) * L * bg::kChannels;
    if (cap * copies * (long long)sizeof(float) <= kMaxLdsBytes) {
      p.tw = c[0]; p.th = c[1];
      p.ntx = (W + p.tw - 1) / p.tw; p.nty = (H + p.th - 1) / p.th;
      p.rowcap = (int)cap;
      return true;
    }
  }
  return false;
}

struct Foot { int vx0, nvx, vy0, nvy; };

__device__ __forceinline__ int cell_of(int i, int size, int n) {
  int i0; float f; bool in;
  bg::axis_cell(bg::pixel_coord(i, size), n, i0, f, in);
  return i0;
}

// vertex columns / rows touched by the tile (the pixel position is monotone in the pixel index)
__device__ __forceinline__ Foot footprint(int tx, int ty, int tw, int th, int W, int H, int GW, int GH) {
  const int xa = tx * tw, xb = min(W, xa + tw) - 1, ya = ty * th, yb = min(H, ya + th) - 1;
  Foot f;
  f.vx0 = cell_of(xa, W, GW);
  f.nvx = cell_of(xb, W, GW) + 2 - f.vx0;
  f.vy0 = cell_of(ya, H, GH);
  f.nvy = cell_of(yb, H, GH) + 2 - f.vy0;
  return f;
}

// footprint slot s <-> (z, jy, ix, c): ((z * nvy + jy) * nvx + ix) * 12 + c
__device__ __forceinline__ void stage_grid(const float* __restrict__ grids, int gi, const Foot& f, int GW, int GH, int L,
                                           int count, float* sg) {
  for (int s = (int)threadIdx.x; s < count; s += kThreads) {
    const int c = s % bg::kChannels;
    int r = s / bg::kChannels;
    const int ix = r % f.nvx; r /= f.nvx;
    const int jy = r % f.nvy;
    const int z = r / f.nvy;
    sg[s] = grids[((((size_t)gi * bg::kChannels + c) * L + z) * GH + (f.vy0 + jy)) * GW + (f.vx0 + ix)];
  }
}

struct StagedGrid {
  const float* sg;
  Foot f;
  __device__ __forceinline__ float operator()(int z, int y, int x, int c) const {
    return sg[((z * f.nvy + (y - f.vy0)) * f.nvx + (x - f.vx0)) * bg::kChannels + c];
  }
};

__device__ __forceinline__ void decode_tile(const TilePlan& p, int& tx, int& ty, int& b) {
  const int wg = (int)blockIdx.x;
  tx = wg % p.ntx;
  ty = (wg / p.ntx) % p.nty;
  b = wg / (p.ntx * p.nty);
}

// ---- forward ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void bilagrid_slice_fwd_kernel(TilePlan p, int H, int W, int G, int GW, int GH,
                                                                       int L, const float* __restrict__ grids,
                                                                       const int* __restrict__ grid_idx,
                                                                       const float* __restrict__ rgb,
                                                                       float* __restrict__ out) {
  extern __shared__ float smem[];
  int tx, ty, b;
  decode_tile(p, tx, ty, b);
  const int gi = grid_idx[b];
  const bool valid = gi >= 0 && gi < G;               // an index outside [0, G) passes the image through
  const Foot f = footprint(tx, ty, p.tw, p.th, W, H, GW, GH);
  const int count = min(f.nvx * f.nvy * L * bg::kChannels, p.rowcap);
  if (valid) stage_grid(grids, gi, f, GW, GH, L, count, smem);
  __syncthreads();
  const StagedGrid v{smem, f};
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int x = tx * p.tw + lane;
  if (lane >= p.tw || x >= W) return;
  for (int r = wave; r < p.th; r += kWaves) {
    const int y = ty * p.th + r;
    if (y >= H) break;
    const size_t px = (((size_t)b * H + y) * W + x) * 3;
    const float c[3] = {rgb[px], rgb[px + 1], rgb[px + 2]};
    float o[3] = {c[0], c[1], c[2]};
    if (valid) bg::slice_pixel(x, y, W, H, c, GW, GH, L, v, o);
    out[px] = o[0]; out[px + 1] = o[1]; out[px + 2] = o[2];
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// LDS: [rowcap] staged grid, then kWaves x [rowcap] per-wave accumulators.  headers[wg] = the tile's footprint (nvx = 0:
// nothing to add), rows[wg * rowcap ..] = its partial row.
__global__ __launch_bounds__(kThreads) void bilagrid_slice_bwd_kernel(TilePlan p, int H, int W, int G, int GW, int GH,
                                                                       int L, const float* __restrict__ grids,
                                                                       const int* __restrict__ grid_idx,
                                                                       const float* __restrict__ rgb,
                                                                       const float* __restrict__ v_out,
                                                                       float* __restrict__ v_rgb,
                                                                       int4* __restrict__ headers,
                                                                       float* __restrict__ rows) {
  extern __shared__ float smem[];
  int tx, ty, b;
  decode_tile(p, tx, ty, b);
  const int gi = grid_idx[b];
  const bool valid = gi >= 0 && gi < G;
  const Foot f = footprint(tx, ty, p.tw, p.th, W, H, GW, GH);
  const int count = min(f.nvx * f.nvy * L * bg::kChannels, p.rowcap);
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (threadIdx.x == 0) headers[blockIdx.x] = valid ? make_int4(f.vx0, f.nvx, f.vy0, f.nvy) : make_int4(0, 0, 0, 0);
  float* sg = smem;
  float* acc = smem + (size_t)p.rowcap * (1 + wave);
  if (valid) stage_grid(grids, gi, f, GW, GH, L, count, sg);
  for (int s = lane; s < count; s += 64) acc[s] = 0.0f;
  __syncthreads();
  const StagedGrid v{sg, f};
  const int x = tx * p.tw + lane;
  const bool col = lane < p.tw && x < W;
  // idle lanes compute on the tile's last pixel (inside the image and inside the staged footprint) and contribute nothing
  const int xc = min(tx * p.tw + min(lane, p.tw - 1), W - 1);
  // which of the 48 sums of a group this lane keeps, and where it goes: (a: z0 / z0+1, i: x0 / x0+1, c)
  const int my_a = lane / 24, my_i = (lane / 12) & 1, my_c = lane % 12;
  for (int r = wave; r < p.th; r += kWaves) {        // uniform per wave
    const int y = ty * p.th + r;
    if (y >= H) break;
    const size_t px = (((size_t)b * H + y) * W + xc) * 3;
    const float c[3] = {rgb[px], rgb[px + 1], rgb[px + 2]};
    const float vo[3] = {v_out[px], v_out[px + 1], v_out[px + 2]};
    if (!valid) {
      if (col) { v_rgb[px] = vo[0]; v_rgb[px + 1] = vo[1]; v_rgb[px + 2] = vo[2]; }
      continue;
    }
    const bg::Cell k = bg::locate(xc, y, W, H, c, GW, GH, L);
    float a0[bg::kChannels], a1[bg::kChannels], A[bg::kChannels], vA[bg::kChannels], vc[3];
    bg::interp_slices(k, v, a0, a1);
    bg::blend_slices(a0, a1, k.fz, A);
    bg::affine_grad(vo, c, vA);
    bg::rgb_grad(A, a0, a1, vA, vo, L, k.zin, vc);
    if (col) { v_rgb[px] = vc[0]; v_rgb[px + 1] = vc[1]; v_rgb[px + 2] = vc[2]; }
    // the row's y cell and weights are the same in every lane
    const int jy = k.y0 - f.vy0;
    const float fy = k.fy;
    const int key = (k.x0 - f.vx0) * L + k.z0;
    unsigned long long remaining = __ballot(col);
    while (remaining) {                               // one pass per (x cell, L cell) present in the row
      const int leader = __ffsll((long long)remaining) - 1;
      const int gkey = __builtin_amdgcn_readlane(key, leader);
      const bool in = col && key == gkey;
      remaining &= ~__ballot(in);
      const float wz0 = in ? 1.0f - k.fz : 0.0f, wz1 = in ? k.fz : 0.0f;
      const float q[4] = {wz0 * (1.0f - k.fx), wz0 * k.fx, wz1 * (1.0f - k.fx), wz1 * k.fx};
      float mine = 0.0f;
#pragma unroll
      for (int ai = 0; ai < 4; ++ai) {
#pragma unroll
        for (int ch = 0; ch < bg::kChannels; ++ch) {
          const float s = gs::wave_sum_uniform(q[ai] * vA[ch]);
          if (lane == ai * bg::kChannels + ch) mine = s;
        }
      }
      if (lane < 48) {
        const int ix = gkey / L + my_i, z = gkey % L + my_a;
        const int s0 = ((z * f.nvy + jy) * f.nvx + ix) * bg::kChannels + my_c;
        const int s1 = s0 + f.nvx * bg::kChannels;
        if (s1 < p.rowcap) {
          acc[s0] += (1.0f - fy) * mine;
          acc[s1] += fy * mine;
        }
      }
    }
  }
  __syncthreads();
  if (!valid) return;
  const float* a = smem + p.rowcap;
  float* row = rows + (size_t)blockIdx.x * p.rowcap;
  for (int s = (int)threadIdx.x; s < count; s += kThreads)
    row[s] = ((a[s] + a[(size_t)p.rowcap + s]) + a[(size_t)2 * p.rowcap + s]) + a[(size_t)3 * p.rowcap + s];
}

// one thread per grid value (channel fastest: neighbouring threads read neighbouring floats of a partial row)
__global__ __launch_bounds__(kThreads) void bilagrid_reduce_kernel(TilePlan p, int B, int H, int W, int G, int GW, int GH,
                                                                    int L, const int* __restrict__ grid_idx,
                                                                    const int4* __restrict__ headers,
                                                                    const float* __restrict__ rows,
                                                                    float* __restrict__ v_grids) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (long long)G * L * GH * GW * bg::kChannels) return;
  const int c = (int)(e % bg::kChannels);
  long long r = e / bg::kChannels;
  const int x = (int)(r % GW); r /= GW;
  const int y = (int)(r % GH); r /= GH;
  const int z = (int)(r % L);
  const int g = (int)(r / L);
  // pixels that can touch vertex x have positions in [x-1, x+1]: a conservative pixel range, two pixels of margin, as
  // tiles; the tile's header decides
  const long long pxa = ((long long)(x - 1) * W) / (GW - 1) - 2, pxb = ((long long)(x + 1) * W + GW - 2) / (GW - 1) + 2;
  const long long pya = ((long long)(y - 1) * H) / (GH - 1) - 2, pyb = ((long long)(y + 1) * H + GH - 2) / (GH - 1) + 2;
  const int txa = x == 0 || pxa < 0 ? 0 : (int)(pxa / p.tw), txb = (int)min((long long)p.ntx - 1, pxb / p.tw);
  const int tya = y == 0 || pya < 0 ? 0 : (int)(pya / p.th), tyb = (int)min((long long)p.nty - 1, pyb / p.th);
  float sum = 0.0f;
  for (int b = 0; b < B; ++b) {
    if (grid_idx[b] != g) continue;
    for (int ty = tya; ty <= tyb; ++ty) {
      for (int tx = txa; tx <= txb; ++tx) {
        const size_t wg = ((size_t)b * p.nty + ty) * p.ntx + tx;
        const int4 h = headers[wg];
        const int ix = x - h.x, jy = y - h.z;
        if (ix < 0 || ix >= h.y || jy < 0 || jy >= h.w) continue;
        const int s = ((z * h.w + jy) * h.y + ix) * bg::kChannels + c;
        if (s < p.rowcap) sum += rows[wg * p.rowcap + s];
      }
    }
  }
  v_grids[((((size_t)g * bg::kChannels + c) * L + z) * GH + y) * GW + x] = sum;
}

// ---- total variation --------------------------------------------------------------------------------------------------
// one thread per grid value: its forward differences go to the value, every difference it takes part in to its own
// gradient (v_grids += weight * d tv).  The value is summed in double: a fixed tree per block, one partial per block,
// then tv_finish_kernel adds the partials in order.
__global__ __launch_bounds__(kThreads) void bilagrid_tv_kernel(long long n, int GW, int GH, int L, float sx, float sy,
                                                                float sz, const float* __restrict__ grids, float weight,
                                                                float* __restrict__ v_grids,
                                                                double* __restrict__ partials) {
  __shared__ double red[kThreads];
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  float value = 0.0f;
  if (e < n) {
    const int x = (int)(e % GW), y = (int)((e / GW) % GH), z = (int)((e / ((long long)GW * GH)) % L);
    const long long sY = GW, sZ = (long long)GW * GH;
    const bool hpx = x > 0, hnx = x + 1 < GW, hpy = y > 0, hny = y + 1 < GH, hpz = z > 0, hnz = z + 1 < L;
    float grad;
    bg::tv_element(grids[e], hpx, hpx ? grids[e - 1] : 0.0f, hnx, hnx ? grids[e + 1] : 0.0f, hpy,
                   hpy ? grids[e - sY] : 0.0f, hny, hny ? grids[e + sY] : 0.0f, hpz, hpz ? grids[e - sZ] : 0.0f, hnz,
                   hnz ? grids[e + sZ] : 0.0f, sx, sy, sz, &value, &grad);
    if (v_grids) v_grids[e] += weight * grad;
  }
  red[threadIdx.x] = (double)value;
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kThreads) void bilagrid_tv_finish_kernel(int blocks, const double* __restrict__ partials,
                                                                       float weight, float* __restrict__ loss_out) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int i = (int)threadIdx.x; i < blocks; i += kThreads) s += partials[i];
  red[threadIdx.x] = s;
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
  }
  if (threadIdx.x == 0) loss_out[0] = (float)((double)weight * red[0]);
}

bool shape_ok(int B, int H, int W, int G, int GW, int GH, int L) {
  if (B < 0 || G < 0 || H < 1 || W < 1 || GW < 2 || GH < 2 || L < 2) return false;
  if ((long long)G * L * GH * GW * bg::kChannels >= (1LL << 31)) return false;
  return true;
}

long long align16(long long v) { return (v + 15) / 16 * 16; }

}  // namespace

// see include/gsdeblur.h
GS_EXPORT int gs_bilagrid_slice_fwd(int B, int H, int W, int G, int GW, int GH, int L, const float* grids,
                                    const int* grid_idx, const float* rgb, float* out, void* stream) {
  if (!shape_ok(B, H, W, G, GW, GH, L)) return GS_ERR_INVALID;
  if (B == 0 || G == 0) return GS_OK;
  if (!grids || !grid_idx || !rgb || !out) return GS_ERR_INVALID;
  TilePlan p;
  if (!make_plan(H, W, GW, GH, L, 1, p)) return GS_ERR_INVALID;
  const long long wgs = (long long)B * p.nty * p.ntx;
  if (wgs >= (1LL << 31)) return GS_ERR_INVALID;
  hipLaunchKernelGGL(bilagrid_slice_fwd_kernel, dim3((unsigned)wgs), dim3(kThreads), (size_t)p.rowcap * sizeof(float),
                     (hipStream_t)stream, p, H, W, G, GW, GH, L, grids, grid_idx, rgb, out);
  return gs_launch_status();
}

// see include/gsdeblur.h
GS_EXPORT long long gs_bilagrid_slice_bwd_workspace_bytes(int B, int H, int W, int G, int GW, int GH, int L) {
  if (!shape_ok(B, H, W, G, GW, GH, L)) return -1;
  if (B == 0 || G == 0) return 0;
  TilePlan p;
  if (!make_plan(H, W, GW, GH, L, 1 + kWaves, p)) return -1;
  const long long wgs = (long long)B * p.nty * p.ntx;
  return align16(wgs * (long long)sizeof(int4)) + wgs * p.rowcap * (long long)sizeof(float);
}

// see include/gsdeblur.h
GS_EXPORT int gs_bilagrid_slice_bwd(int B, int H, int W, int G, int GW, int GH, int L, const float* grids,
                                    const int* grid_idx, const float* rgb, const float* v_out, float* v_rgb,
                                    float* v_grids, void* ws, long long ws_bytes, void* stream) {
  if (!shape_ok(B, H, W, G, GW, GH, L)) return GS_ERR_INVALID;
  if (B == 0 || G == 0) return GS_OK;
  if (!grids || !grid_idx || !rgb || !v_out || !v_rgb || !v_grids || !ws) return GS_ERR_INVALID;
  if ((uintptr_t)ws & 15) return GS_ERR_INVALID;
  TilePlan p;
  if (!make_plan(H, W, GW, GH, L, 1 + kWaves, p)) return GS_ERR_INVALID;
  const long long wgs = (long long)B * p.nty * p.ntx;
  if (wgs >= (1LL << 31)) return GS_ERR_INVALID;
  const long long head_bytes = align16(wgs * (long long)sizeof(int4));
  if (ws_bytes < head_bytes + wgs * p.rowcap * (long long)sizeof(float)) return GS_ERR_WORKSPACE;
  int4* headers = reinterpret_cast<int4*>(ws);
  float* rows = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + head_bytes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bilagrid_slice_bwd_kernel, dim3((unsigned)wgs), dim3(kThreads),
                     (size_t)p.rowcap * (1 + kWaves) * sizeof(float), st, p, H, W, G, GW, GH, L, grids, grid_idx, rgb,
                     v_out, v_rgb, headers, rows);
  int status = gs_launch_status();
  if (status != GS_OK) return status;
  const long long n = (long long)G * L * GH * GW * bg::kChannels;
  hipLaunchKernelGGL(bilagrid_reduce_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, p, B,
                     H, W, G, GW, GH, L, grid_idx, headers, rows, v_grids);
  return gs_launch_status();
}

// see include/gsdeblur.h
GS_EXPORT long long gs_bilagrid_tv_workspace_bytes(int G, int GW, int GH, int L) {
  if (!shape_ok(0, 1, 1, G, GW, GH, L)) return -1;
  const long long n = (long long)G * L * GH * GW * bg::kChannels;
  return (n + kThreads - 1) / kThreads * (long long)sizeof(double);
}

// see include/gsdeblur.h
GS_EXPORT int gs_bilagrid_tv_fwd_bwd(int G, int GW, int GH, int L, const float* grids, float weight, float* loss_out,
                                     float* v_grids, void* ws, long long ws_bytes, void* stream) {
  if (!shape_ok(0, 1, 1, G, GW, GH, L)) return GS_ERR_INVALID;
  if (G == 0) return GS_OK;
  if (!grids || !loss_out || !ws) return GS_ERR_INVALID;
  if ((uintptr_t)ws & 7) return GS_ERR_INVALID;
  const long long n = (long long)G * L * GH * GW * bg::kChannels;
  const long long blocks = (n + kThreads - 1) / kThreads;
  if (ws_bytes < blocks * (long long)sizeof(double)) return GS_ERR_WORKSPACE;
  const long long planes = (long long)G * bg::kChannels;
  const float sx = bg::tv_axis_scale(planes * L * GH * (GW - 1));
  const float sy = bg::tv_axis_scale(planes * L * (GH - 1) * GW);
  const float sz = bg::tv_axis_scale(planes * (L - 1) * GH * GW);
  double* partials = reinterpret_cast<double*>(ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bilagrid_tv_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, n, GW, GH, L, sx, sy, sz, grids,
                     weight, v_grids, partials);
  int status = gs_launch_status();
  if (status != GS_OK) return status;
  hipLaunchKernelGGL(bilagrid_tv_finish_kernel, dim3(1), dim3(kThreads), 0, st, (int)blocks, partials, weight, loss_out);
  return gs_launch_status();
}
