// blur.hip — per-frame blur statistics of a point cloud under the motion model (blurscore.py): F frames x N points
// pairs, each a projection and a pixel velocity, reduced to five numbers per frame.  Math: blur_math.h.  gfx950, wave64.
//
// Two launches, nothing is read back between them:
//   1. pairs: grid (chunks of kChunk points, groups of kFrameGroup frames).  A thread loads PPT points of its chunk into
//      registers once and loops over the frames of its group.  A frame's constants (V, lin, ang, fx fy cx cy, E T) are
//      indexed by blockIdx.y and the loop counter alone: they come through the scalar cache (s_load_dwordx*), not
//      through vector loads.  Per frame the wave's partials are added in a butterfly and lane 0 leaves them in LDS; after
//      the loop thread g adds the waves of frame g in order and stores one row of partials[chunk][frame];
//   2. finish: one wave per frame; lane l adds the rows of chunks l, l + 64, ... in order, the lanes are added in the
//      same butterfly, lane 0 divides and stores.
// No atomics; the order of every sum depends on N (and on the points per thread, a compile-time choice) alone, so two
// runs agree bit for bit.  kChunk is fixed, so the workspace and the partials' layout do not depend on PPT: a thread block
// is kChunk / PPT threads.
#include "gs_common.h"
#include "blur_math.h"

namespace {

namespace bl = gs::blur;

constexpr int kDefaultPointsPerThread = 4;        // DESIGN 5.12 has the sweep
constexpr int kFinishThreads = 256;               // pass 2: four frames per workgroup
constexpr int kMaxFrames = 65535 * bl::kFrameGroup;
constexpr int kMaxPoints = 1 << 30;

static_assert(sizeof(bl::Partial) == 32, "partials rows are 32 bytes");

__device__ __forceinline__ void wave_add(bl::Partial& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bl::Partial b;
    b.sum_blur = __shfl_xor(a.sum_blur, o);
    b.sum_sq = __shfl_xor(a.sum_sq, o);
    b.sum_skew = __shfl_xor(a.sum_skew, o);
    b.max_blur = __shfl_xor(a.max_blur, o);
    b.count = __shfl_xor(a.count, o);
    bl::add_partial(a, b);
  }
}

// partials [chunks][F]
template <int PPT>
__global__ __launch_bounds__(bl::kChunk / PPT) void blur_pairs_kernel(int F, int N, const float* __restrict__ points,
                                                                       const float* __restrict__ viewmats,
                                                                       const float* __restrict__ lin,
                                                                       const float* __restrict__ ang,
                                                                       const float* __restrict__ intrins,
                                                                       const float* __restrict__ times, float W, float H,
                                                                       float clip, bl::Partial* __restrict__ partials) {
  constexpr int kThreads = bl::kChunk / PPT, kWaves = kThreads / gs::kWave;
  static_assert(kThreads % gs::kWave == 0 && kThreads >= bl::kFrameGroup, "block shape");
  __shared__ bl::Partial wave_part[bl::kFrameGroup * kWaves];
  const int t = (int)threadIdx.x, chunk = (int)blockIdx.x;
  const int f0 = (int)blockIdx.y * bl::kFrameGroup;
  const int nf = F - f0 < bl::kFrameGroup ? F - f0 : bl::kFrameGroup;
  float p[PPT][3];
  bool have[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const long long i = (long long)chunk * bl::kChunk + j * kThreads + t;
    have[j] = i < N;
    const float* q = points + (have[j] ? i : 0) * 3;
    p[j][0] = q[0]; p[j][1] = q[1]; p[j][2] = q[2];
  }
  for (int g = 0; g < nf; ++g) {                          // uniform per workgroup
    const int f = f0 + g;
    const bl::Frame fr = {viewmats + (size_t)f * 16, lin + (size_t)f * 3, ang + (size_t)f * 3,
                          intrins[(size_t)f * 4], intrins[(size_t)f * 4 + 1], intrins[(size_t)f * 4 + 2],
                          intrins[(size_t)f * 4 + 3], times[(size_t)f * 2], times[(size_t)f * 2 + 1]};
    bl::Partial a;
    bl::clear_partial(a);
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      float blur, skew;
      const bool visible = bl::pair_blur(fr, p[j], W, H, clip, &blur, &skew) && have[j];
      bl::add_pair(a, visible, blur, skew);
    }
    wave_add(a);
    if (gs::lane_id() == 0) wave_part[g * kWaves + t / gs::kWave] = a;
  }
  __syncthreads();
  if (t < nf) {
    bl::Partial a = wave_part[t * kWaves];
    for (int w = 1; w < kWaves; ++w) bl::add_partial(a, wave_part[t * kWaves + w]);
    partials[(size_t)chunk * F + f0 + t] = a;
  }
}

__global__ __launch_bounds__(kFinishThreads) void blur_finish_kernel(int F, int chunks,
                                                                      const bl::Partial* __restrict__ partials,
                                                                      int* __restrict__ counts, float* __restrict__ stats) {
  const int f = (int)blockIdx.x * (kFinishThreads / gs::kWave) + (int)threadIdx.x / gs::kWave;
  if (f >= F) return;                                     // a whole wave leaves; no barrier below
  bl::Partial a;
  bl::clear_partial(a);
  for (int c = gs::lane_id(); c < chunks; c += gs::kWave) bl::add_partial(a, partials[(size_t)c * F + f]);
  wave_add(a);
  if (gs::lane_id() == 0) {
    int count;
    float s[4];
    bl::finish(a, &count, s);
    counts[f] = count;
    stats[(size_t)f * 4] = s[0]; stats[(size_t)f * 4 + 1] = s[1]; stats[(size_t)f * 4 + 2] = s[2];
    stats[(size_t)f * 4 + 3] = s[3];
  }
}

bool shape_ok(int F, int N) { return F >= 0 && F <= kMaxFrames && N >= 0 && N <= kMaxPoints; }

int chunks_of(int N) { return (N + bl::kChunk - 1) / bl::kChunk; }

template <int PPT>
int run(int F, int N, const float* points, const float* viewmats, const float* lin, const float* ang,
        const float* intrins, const float* times, int W, int H, float clip, int* counts, float* stats,
        bl::Partial* partials, hipStream_t st) {
  const int chunks = chunks_of(N);
  const unsigned groups = (unsigned)((F + bl::kFrameGroup - 1) / bl::kFrameGroup);
  hipLaunchKernelGGL((blur_pairs_kernel<PPT>), dim3((unsigned)chunks, groups), dim3(bl::kChunk / PPT), 0, st, F, N, points,
                     viewmats, lin, ang, intrins, times, (float)W, (float)H, clip, partials);
  int status = gs_launch_status();
  if (status != GS_OK) return status;
  constexpr int per_block = kFinishThreads / gs::kWave;
  hipLaunchKernelGGL(blur_finish_kernel, dim3((unsigned)((F + per_block - 1) / per_block)), dim3(kFinishThreads), 0, st, F,
                     chunks, partials, counts, stats);
  return gs_launch_status();
}

}  // namespace

// see include/gsdeblur.h
GS_EXPORT long long gs_blur_stats_workspace_bytes(int F, int N) {
  if (!shape_ok(F, N)) return -1;
  return (long long)chunks_of(N) * F * (long long)sizeof(bl::Partial);
}

// see include/gsdeblur.h
GS_EXPORT int gs_blur_stats_ppt(int F, int N, const float* points, const float* viewmats, const float* lin,
                                const float* ang, const float* intrins, const float* times, int W, int H, float clip,
                                int points_per_thread, int* counts, float* stats, void* ws, long long ws_bytes,
                                void* stream) {
  if (!shape_ok(F, N) || W < 1 || H < 1 || !(clip == clip)) return GS_ERR_INVALID;
  if (F == 0) return GS_OK;
  if (!counts || !stats) return GS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {                                           // no pair: zeros, and no kernel
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)F * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)F * 4 * sizeof(float), st);
    return e == hipSuccess ? GS_OK : 1000 + (int)e;
  }
  if (!points || !viewmats || !lin || !ang || !intrins || !times || !ws || ((uintptr_t)ws & 7)) return GS_ERR_INVALID;
  if (ws_bytes < gs_blur_stats_workspace_bytes(F, N)) return GS_ERR_WORKSPACE;
  bl::Partial* partials = reinterpret_cast<bl::Partial*>(ws);
  switch (points_per_thread > 0 ? points_per_thread : kDefaultPointsPerThread) {
#define BLUR_CASE(P) \
  case P: return run<P>(F, N, points, viewmats, lin, ang, intrins, times, W, H, clip, counts, stats, partials, st)
    BLUR_CASE(1); BLUR_CASE(2); BLUR_CASE(4); BLUR_CASE(8); BLUR_CASE(16);
#undef BLUR_CASE
  }
  return GS_ERR_INVALID;
}

// see include/gsdeblur.h
GS_EXPORT int gs_blur_stats(int F, int N, const float* points, const float* viewmats, const float* lin, const float* ang,
                            const float* intrins, const float* times, int W, int H, float clip, int* counts,
                            float* stats, void* ws, long long ws_bytes, void* stream) {
  return gs_blur_stats_ppt(F, N, points, viewmats, lin, ang, intrins, times, W, H, clip, 0, counts, stats, ws, ws_bytes,
                           stream);
}
