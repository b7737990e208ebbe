// colorcorrect.hip — colour-corrected evaluation metrics (colorcorrect.py): the rendered image is fitted to the ground
// truth by a per-channel quadratic colour warp, num_iters times.  Math: colorcorrect_math.h.  gfx950, wave64.
//
// One iteration is three launches, nothing is read back between them:
//   1. moments: per image and output channel the masked normal equations, 3 x 65 float64 sums over all pixels.  198
//      accumulators do not fit a thread's registers, so the layout is output-stationary: a workgroup stages a tile of
//      kTile pixels in LDS — (r, g, b, 1, ref_0, ref_1, ref_2) as doubles and the three mask bits — and thread t < 195
//      owns ONE sum, channel t / 65, and walks the tile: four 8-byte LDS reads (the slots of its term; the lanes of a
//      wave read the same 64-byte record, no bank conflict) and one mask word per pixel.  Workgroup j of an image takes
//      tiles j, j + n, j + 2n, ... in that order and stores one partial row;
//   2. solve: one workgroup per (image, channel) adds the partial rows in a fixed order (eight interleaved parts per sum,
//      then the parts) and one thread solves the 10 x 10 system (solve_channel, degenerate rule included);
//   3. apply: one thread per pixel, x <- clip(a . W) stored as float32, in place from the second iteration on.
// No float atomics; the order of every sum depends on (H, W) alone, so two runs agree bit for bit and an image's result
// does not depend on what else is in the batch.
#include "gs_common.h"
#include "colorcorrect_math.h"

namespace {

namespace cc = gs::colorcorrect;

constexpr int kThreads = 256;
constexpr int kTile = 256;                        // pixels staged per pass: one per thread
constexpr int kRow = 3 * cc::kSums;               // 195 sums per image
constexpr int kRecord = 8;                        // doubles per staged pixel (kSlots, padded)
constexpr int kMaxGroups = 1024;                  // moments workgroups per image: four per CU for a single image
constexpr int kSolveThreads = 512;
constexpr int kSolveParts = 8;                    // threads that share one sum's partial rows in the solve kernel

static_assert(kRow <= kThreads && cc::kSlots <= kRecord && kTile == kThreads, "layout");

int groups_per_image(long long pixels) {
  const long long tiles = (pixels + kTile - 1) / kTile;
  return (int)(tiles < kMaxGroups ? tiles : kMaxGroups);
}

// partials [B][groups][kRow]
__global__ __launch_bounds__(kThreads) void color_correct_moments_kernel(long long pixels, int groups, float lo, float hi,
                                                                          const float* __restrict__ img,
                                                                          const float* __restrict__ x,
                                                                          const float* __restrict__ ref,
                                                                          double* __restrict__ partials) {
  __shared__ double rec[kTile * kRecord];
  __shared__ unsigned masks[kTile];
  const int t = (int)threadIdx.x, j = (int)blockIdx.x, b = (int)blockIdx.y;
  const size_t base = (size_t)b * (size_t)pixels * 3;
  const bool owner = t < kRow;
  const int c = owner ? t / cc::kSums : 0;
  int s[4];
  cc::sum_slots(owner ? t % cc::kSums : 0, c, s);
  double acc = 0.0;
  const long long tiles = (pixels + kTile - 1) / kTile;
  for (long long tile = j; tile < tiles; tile += groups) {          // uniform per workgroup
    const long long p = tile * kTile + t;
    double* r = rec + t * kRecord;
    if (p < pixels) {
      const size_t o = base + (size_t)p * 3;
      const float pi[3] = {img[o], img[o + 1], img[o + 2]};
      const float px[3] = {x[o], x[o + 1], x[o + 2]};
      const float pr[3] = {ref[o], ref[o + 1], ref[o + 2]};
      r[0] = (double)px[0]; r[1] = (double)px[1]; r[2] = (double)px[2]; r[cc::kSlotOne] = 1.0;
      r[cc::kSlotRef] = (double)pr[0]; r[cc::kSlotRef + 1] = (double)pr[1]; r[cc::kSlotRef + 2] = (double)pr[2];
      masks[t] = cc::row_masks(pi, px, pr, lo, hi);
    } else {
      masks[t] = 0u;                                                // past the image: the record is never read
    }
    __syncthreads();
    const long long left = pixels - tile * kTile;
    const int n = left < kTile ? (int)left : kTile;
    if (owner) {
      for (int q = 0; q < n; ++q) {
        const double* v = rec + q * kRecord;
        const double term = (v[s[0]] * v[s[1]]) * (v[s[2]] * v[s[3]]);
        if ((masks[q] >> c) & 1u) acc += term;
      }
    }
    __syncthreads();
  }
  if (owner) partials[((size_t)b * groups + j) * kRow + t] = acc;
}

// grid (3, B).  warp [B][3][10] is what the apply pass reads; warps_out (nullable) [B][num_iters][3][10] keeps every
// iteration's
__global__ __launch_bounds__(kSolveThreads) void color_correct_solve_kernel(int groups, int iter, int num_iters,
                                                                             const double* __restrict__ partials,
                                                                             double* __restrict__ warp,
                                                                             double* __restrict__ warps_out) {
  __shared__ double part[kSolveParts * cc::kSums];
  __shared__ double sums[cc::kSums];
  __shared__ double L[cc::kFeatures * cc::kFeatures];
  __shared__ double d[cc::kFeatures];
  __shared__ double w[cc::kFeatures];
  const int c = (int)blockIdx.x, b = (int)blockIdx.y;
  // up to 1024 dependent reads per sum are latency, not bandwidth: kSolveParts threads share a sum, thread q of them adds
  // rows q, q + kSolveParts, ... in order, then the parts are added in order
  for (int slot = (int)threadIdx.x; slot < kSolveParts * cc::kSums; slot += kSolveThreads) {
    const int k = slot % cc::kSums, q = slot / cc::kSums;
    const double* p = partials + (size_t)b * groups * kRow + c * cc::kSums + k;
    double sum = 0.0;
    for (int g = q; g < groups; g += kSolveParts) sum += p[(size_t)g * kRow];
    part[slot] = sum;
  }
  __syncthreads();
  if ((int)threadIdx.x < cc::kSums) {
    double sum = 0.0;
    for (int q = 0; q < kSolveParts; ++q) sum += part[q * cc::kSums + threadIdx.x];
    sums[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) cc::solve_channel(sums, c, L, d, w);
  __syncthreads();
  if ((int)threadIdx.x < cc::kFeatures) {
    const double v = w[threadIdx.x];
    warp[((size_t)b * 3 + c) * cc::kFeatures + threadIdx.x] = v;
    if (warps_out) warps_out[(((size_t)b * num_iters + iter) * 3 + c) * cc::kFeatures + threadIdx.x] = v;
  }
}

// grid (ceil(pixels / kThreads), B); x and out may be the same buffer
__global__ __launch_bounds__(kThreads) void color_correct_apply_kernel(long long pixels, const double* __restrict__ warp,
                                                                        const float* x, float* out) {
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= pixels) return;
  const int b = (int)blockIdx.y;
  const size_t o = ((size_t)b * (size_t)pixels + (size_t)p) * 3;
  const float px[3] = {x[o], x[o + 1], x[o + 2]};
  float y[3];
  cc::apply_warp(px, warp + (size_t)b * 3 * cc::kFeatures, y);
  out[o] = y[0]; out[o + 1] = y[1]; out[o + 2] = y[2];
}

bool shape_ok(int B, int H, int W) {
  return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= (1LL << 30);
}

long long warp_bytes(int B) { return (long long)B * 3 * cc::kFeatures * (long long)sizeof(double); }

}  // namespace

// see include/gsdeblur.h
GS_EXPORT long long gs_color_correct_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W)) return -1;
  return warp_bytes(B) + (long long)B * groups_per_image((long long)H * W) * kRow * (long long)sizeof(double);
}

// see include/gsdeblur.h
GS_EXPORT int gs_color_correct(int B, int H, int W, const float* img, const float* ref, int num_iters, double eps,
                               float* out, double* warps, void* ws, long long ws_bytes, void* stream) {
  if (!shape_ok(B, H, W) || num_iters < 0) return GS_ERR_INVALID;
  if (B == 0) return GS_OK;
  if (!img || !ref || !out || !ws || out == img || out == ref) return GS_ERR_INVALID;
  if ((uintptr_t)ws & 7) return GS_ERR_INVALID;
  if (ws_bytes < gs_color_correct_workspace_bytes(B, H, W)) return GS_ERR_WORKSPACE;
  const long long pixels = (long long)H * W;
  const int groups = groups_per_image(pixels);
  hipStream_t st = (hipStream_t)stream;
  if (num_iters == 0) {
    const hipError_t e = hipMemcpyAsync(out, img, (size_t)B * pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? GS_OK : 1000 + (int)e;
  }
  double* warp = reinterpret_cast<double*>(ws);
  double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + warp_bytes(B));
  const float lo = (float)eps, hi = (float)(1.0 - eps);
  const unsigned apply_blocks = (unsigned)((pixels + kThreads - 1) / kThreads);
  for (int it = 0; it < num_iters; ++it) {
    const float* x = it == 0 ? img : out;
    hipLaunchKernelGGL(color_correct_moments_kernel, dim3((unsigned)groups, (unsigned)B), dim3(kThreads), 0, st, pixels,
                       groups, lo, hi, img, x, ref, partials);
    int status = gs_launch_status();
    if (status != GS_OK) return status;
    hipLaunchKernelGGL(color_correct_solve_kernel, dim3(3, (unsigned)B), dim3(kSolveThreads), 0, st, groups, it, num_iters,
                       partials, warp, warps);
    status = gs_launch_status();
    if (status != GS_OK) return status;
    hipLaunchKernelGGL(color_correct_apply_kernel, dim3(apply_blocks, (unsigned)B), dim3(kThreads), 0, st, pixels, warp, x,
                       out);
    status = gs_launch_status();
    if (status != GS_OK) return status;
  }
  return GS_OK;
}
